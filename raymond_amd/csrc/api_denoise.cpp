// C-ABI implementation (include/raymond_hip.h) of the denoise entry points, rmd_despike, rmd_despike_dual, rmd_tile_luma_error, rmd_tile_weighted_error,
// rmd_tile_weighted_error_dual, rmd_tile_error and rmd_tile_error_dual.  Host code only; the kernels are in denoise*.hip, despike.hip, despike_dual.hip, tile_luma.hip,
// tile_weighted.hip, tile_weighted_dual.hip and, rmd_tile_error's, kernels.hip.
// Every entry point is its argument checks in its own order and then, inside rmd::guarded: the rect checks, the context, one carved scratch block
// (denoise_host.hpp has the layouts), one upload of the rects, its launcher (launch.hpp) and the wait.
#define RMD_WITH_HIP 1
#include <hip/hip_runtime.h> // (tile_reduce.hpp's combine, which the rule headers bring along under hipcc, names the device runtime)

#include "despike_rule.hpp"
#include "internal.hpp"
#include "launch.hpp"
#include "tile_luma_rule.hpp"
#include "tile_weighted_dual_rule.hpp"
#include "tile_weighted_rule.hpp"

namespace rmd {
// Rects inside the frame and pairwise disjoint (rects without pixels cover nothing): sorted by left edge, each rect is compared with the ones that
// start before it ends.
bool denoise_rects_ok(const rmd_tile_rect *rects, uint32_t n_rects, uint32_t width, uint32_t height, const char **why) {
	// (*why: the rule that was broken; the caller puts its own name in front)
	if (!rects_inside(rects, n_rects, width, height)) return *why = kRectOutside, false;
	std::vector<uint32_t> order;
	for (uint32_t i = 0; i < n_rects; i++)
		if (rects[i].width != 0 && rects[i].height != 0) order.push_back(i);
	std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rects[a].left < rects[b].left; });
	for (size_t i = 0; i < order.size(); i++) {
		const rmd_tile_rect &a = rects[order[i]];
		for (size_t j = i + 1; j < order.size() && rects[order[j]].left < (uint64_t)a.left + a.width; j++) {
			const rmd_tile_rect &b = rects[order[j]];
			if (b.top < (uint64_t)a.top + a.height && a.top < (uint64_t)b.top + b.height) return *why = "tile rectangles overlap", false;
		}
	}
	return true;
}
} // namespace rmd

namespace {
using rmd::DenoiseInput;
using rmd::DenoiseWeights;
using rmd::any_overlap;
using rmd::fail;
constexpr rmd_status kInvalid = RMD_ERR_INVALID_ARGUMENT;

// ---------------------------------------------------------------- the argument checks (`name`: the entry point's name and ": ", the messages' prefix)
// Until the upload `in` holds the caller's own arguments: rects and counts are host memory
rmd_status check_frame(rmd_context *ctx, const std::string &name, const DenoiseInput &in, bool dual, const double *out_dev) {
	if (!in.accum_a || !in.accum_sq_a || (dual && (!in.accum_b || !in.accum_sq_b)) || !out_dev || in.W == 0 || in.H == 0 ||
	    (in.n_rects && (!in.rects || !in.counts_a || (dual && !in.counts_b))))
		return fail(ctx, kInvalid, name + "bad argument");
	return RMD_OK;
}
rmd_status check_features(rmd_context *ctx, const std::string &name, const DenoiseInput &in, bool with_counts) {
	if ((in.feat == nullptr) != (in.feat_sq == nullptr)) return fail(ctx, kInvalid, name + "feat_dev and feat_sq_dev must both be given or both be NULL");
	if (with_counts && in.feat && in.n_rects && !in.counts_f) return fail(ctx, kInvalid, name + "rect_counts_f is NULL with n_rects > 0");
	return RMD_OK;
}
rmd_status check_window(rmd_context *ctx, const std::string &name, uint32_t radius, uint32_t patch_radius) {
	if (radius > rmd::kDenoiseMaxRadius) return fail(ctx, kInvalid, name + "radius must be <= 12");
	if (patch_radius > rmd::kDenoiseMaxPatch) return fail(ctx, kInvalid, name + "patch_radius must be <= 4");
	return RMD_OK;
}
rmd_status check_levels(rmd_context *ctx, const std::string &name, uint32_t levels) {
	return levels > rmd::kAtrousMaxLevels ? fail(ctx, kInvalid, name + "levels must be <= 8") : RMD_OK;
}
rmd_status check_weights(rmd_context *ctx, const std::string &name, double k, double alpha) {
	if (!(k > 0.0) || !std::isfinite(k)) return fail(ctx, kInvalid, name + "k must be finite and > 0");
	if (!(alpha >= 0.0) || !std::isfinite(alpha)) return fail(ctx, kInvalid, name + "alpha must be finite and >= 0");
	return RMD_OK;
}
rmd_status check_feature_weights(rmd_context *ctx, const std::string &name, double k_f, double tau) {
	if (!(k_f > 0.0) || !std::isfinite(k_f)) return fail(ctx, kInvalid, name + "k_f must be finite and > 0");
	if (!(tau > 0.0) || !std::isfinite(tau)) return fail(ctx, kInvalid, name + "tau must be finite and > 0");
	return RMD_OK;
}
rmd_status check_slope(rmd_context *ctx, const std::string &name, double slope) { // (the _slope calls; the others pass 0)
	return !(slope >= 0.0) || !std::isfinite(slope) ? fail(ctx, kInvalid, name + "slope must be finite and >= 0") : RMD_OK;
}
rmd_status check_rects(rmd_context *ctx, const std::string &name, const rmd_tile_rect *rects, uint32_t n_rects, uint32_t width, uint32_t height) {
	const char *why = nullptr;
	return rmd::denoise_rects_ok(rects, n_rects, width, height, &why) ? RMD_OK : fail(ctx, kInvalid, name + why);
}

// The caller's frame as the checks and the upload take it: the single-buffer forms have one pair of sums and one count array, the dual forms two and,
// with features, the features' counts.  count_image_columns is set by the upload
DenoiseInput single_input(const double *accum, const double *accum_sq, const double *feat, const double *feat_sq, uint32_t width, uint32_t height,
                          const rmd_tile_rect *rects, const uint32_t *counts, uint32_t n_rects) {
	DenoiseInput in{};
	in.accum_a = accum, in.accum_sq_a = accum_sq, in.feat = feat, in.feat_sq = feat_sq;
	in.rects = rects, in.counts_a = counts, in.n_rects = n_rects, in.W = width, in.H = height;
	return in;
}
DenoiseInput dual_input(const double *accum_a, const double *accum_sq_a, const double *accum_b, const double *accum_sq_b, const double *feat, const double *feat_sq,
                        uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *counts_a, const uint32_t *counts_b, const uint32_t *counts_f,
                        uint32_t n_rects) {
	DenoiseInput in = single_input(accum_a, accum_sq_a, feat, feat_sq, width, height, rects, counts_a, n_rects);
	in.accum_b = accum_b, in.accum_sq_b = accum_sq_b, in.counts_b = counts_b, in.counts_f = counts_f;
	return in;
}

// ---------------------------------------------------------------- scratch, upload, wait
// One call's device scratch: the block (the call's own, freed when it returns; `keep`: the context's, grown when a call needs more) and its parts
struct Scratch {
	rmd::DeviceBuffer own;
	rmd::ScratchLayout layout;
	unsigned char *base = nullptr;
	rmd_status carve(rmd_context *ctx, const rmd::ScratchLayout &L, rmd::DeviceBuffer *keep = nullptr) {
		RMD_HIP(ctx, keep ? keep->grow(L.total) : own.alloc(L.total));
		layout = L, base = (keep ? keep : &own)->as<unsigned char>();
		return RMD_OK;
	}
	template <class T>
	T *part(rmd::ScratchPart p) const { return layout.used[p] ? reinterpret_cast<T *>(base + layout.offset[p]) : nullptr; }
};
// The rects and the counts the block has parts for go to the device on the context's stream (n_rects = 0: nothing is copied); `in` then holds the device
// pointers, and the columns of the count image: each rect gets a column of 256-thread workgroups that covers the largest rect, 1 .. 1,024
rmd_status upload_rects(rmd_context *ctx, const Scratch &s, DenoiseInput &in) {
	rmd_tile_rect *d_rects = s.part<rmd_tile_rect>(rmd::kPartRects);
	const uint32_t *h_counts[3] = {in.counts_a, in.counts_b, in.counts_f};
	uint32_t *d_counts[3] = {s.part<uint32_t>(rmd::kPartCountsA), s.part<uint32_t>(rmd::kPartCountsB), s.part<uint32_t>(rmd::kPartCountsF)};
	uint64_t largest = 0;
	for (uint32_t i = 0; i < in.n_rects; i++) largest = std::max<uint64_t>(largest, (uint64_t)in.rects[i].width * in.rects[i].height);
	if (in.n_rects != 0) {
		RMD_HIP(ctx, hipMemcpyAsync(d_rects, in.rects, (size_t)in.n_rects * sizeof(rmd_tile_rect), hipMemcpyHostToDevice, ctx->stream));
		for (int i = 0; i < 3; i++)
			if (d_counts[i]) RMD_HIP(ctx, hipMemcpyAsync(d_counts[i], h_counts[i], (size_t)in.n_rects * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
	}
	in.rects = d_rects, in.counts_a = d_counts[0], in.counts_b = d_counts[1], in.counts_f = d_counts[2];
	in.count_image_columns = (uint32_t)std::min<uint64_t>(1024u, std::max<uint64_t>(1u, (largest + 255u) / 256u));
	return RMD_OK;
}
// Every call ends with the wait (host arrays and the block are read by copies and kernels until here) and reports a fault: the sums came from launches
// this call has waited for
rmd_status finish(rmd_context *ctx) {
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return rmd::check_fault(ctx);
}

// ---------------------------------------------------------------- the single-buffer filters (denoise.hip, denoise_atrous.hip)
// rmd_denoise and rmd_denoise_guided[_slope] (levels null), rmd_denoise_atrous[_slope] (levels given; radius and patch_radius unused).  `what`: the entry point's name
rmd_status denoise_single(const char *what, rmd_context *ctx, DenoiseInput in, const uint32_t *levels, uint32_t radius, uint32_t patch_radius, const DenoiseWeights &w,
                          double *out_dev) {
	const std::string name = std::string(what) + ": ";
	const bool guided = in.feat != nullptr;
	if (rmd_status s = check_frame(ctx, name, in, false, out_dev)) return s;
	if (rmd_status s = check_features(ctx, name, in, false)) return s;
	// no two of the three W*H*3-double ranges overlap; nor do the two W*H*7-double feature ranges, each other or out_dev's
	const unsigned __int128 bytes = (unsigned __int128)in.W * in.H * 3u * sizeof(double), fbytes = (unsigned __int128)in.W * in.H * RMD_FEATURE_CHANNELS * sizeof(double);
	if (any_overlap({{in.accum_a, bytes}, {in.accum_sq_a, bytes}, {out_dev, bytes}})) return fail(ctx, kInvalid, name + "accum_dev, accum_sq_dev and out_dev must not alias");
	if (any_overlap({{in.feat, fbytes}, {in.feat_sq, fbytes}, {out_dev, bytes}})) return fail(ctx, kInvalid, name + "feat_dev, feat_sq_dev and out_dev must not alias");
	if (rmd_status s = levels ? check_levels(ctx, name, *levels) : check_window(ctx, name, radius, patch_radius)) return s;
	if (rmd_status s = check_weights(ctx, name, w.k, w.alpha)) return s;
	if (guided) {
		if (rmd_status s = check_feature_weights(ctx, name, w.k_f, w.tau)) return s;
		if (rmd_status s = check_slope(ctx, name, w.slope)) return s;
	}
	const bool sloped = guided && w.slope > 0.0;
	return rmd::guarded(ctx, what, [&] {
		if (rmd_status s = check_rects(ctx, name, in.rects, in.n_rects, in.W, in.H)) return s;
		if (rmd_status s = rmd::bind(ctx)) return s;
		Scratch sc;
		if (rmd_status s = sc.carve(ctx, rmd::denoise_scratch_layout(levels ? rmd::kScratchAtrous : rmd::kScratchSingle, in.W, in.H, in.n_rects, guided, 0u, 0u, sloped && !levels, sloped && levels))) return s;
		if (rmd_status s = upload_rects(ctx, sc, in)) return s;
		uint32_t *n_img = sc.part<uint32_t>(rmd::kPartCountImg);
		double *feat_planes = sc.part<double>(rmd::kPartFeatPlanes);
		if (levels) RMD_HIP(ctx, rmd::launch_denoise_atrous(ctx->stream, in, w, *levels, n_img, sc.part<double>(rmd::kPartPlanes), feat_planes, sc.part<double>(rmd::kPartSlopePlanes), out_dev));
		else RMD_HIP(ctx, rmd::launch_denoise_guided(ctx->stream, in, w, radius, patch_radius, n_img, feat_planes, sc.part<double>(rmd::kPartSlopePlanes), out_dev));
		return finish(ctx);
	});
}

// ---------------------------------------------------------------- the dual-buffer filters (denoise_dual.hip, denoise_atrous_dual.hip)
// rmd_denoise_dual and its guided and region forms (levels null), rmd_denoise_atrous_dual[_slope] and their region forms (levels given; radius and patch_radius
// unused).  `regional`: a region form, which writes the pixels of its n_region rects only; its region may still be NULL when n_region is 0.  Without
// features rect_counts_f, k_f, tau and the slope (the _slope calls: w.slope, 0 in every other) are not read
rmd_status denoise_dual(const char *what, bool regional, rmd_context *ctx, DenoiseInput in, const rmd_tile_rect *region, uint32_t n_region, const uint32_t *levels,
                        uint32_t radius, uint32_t patch_radius, const DenoiseWeights &w, double *out_dev, double *err_dev) {
	const std::string name = std::string(what) + ": ";
	const bool guided = in.feat != nullptr;
	if (rmd_status s = check_frame(ctx, name, in, true, out_dev)) return s;
	if (regional && n_region && !region) return fail(ctx, kInvalid, name + "region is NULL with n_region > 0");
	if (rmd_status s = check_features(ctx, name, in, true)) return s;
	// no two of the six ranges overlap: five of W*H*3 doubles, err_dev's W*H; nor do the two W*H*7-double feature ranges, each other or any of the six
	const unsigned __int128 bytes = (unsigned __int128)in.W * in.H * 3u * sizeof(double), fbytes = (unsigned __int128)in.W * in.H * RMD_FEATURE_CHANNELS * sizeof(double);
	if (any_overlap({{in.accum_a, bytes}, {in.accum_sq_a, bytes}, {in.accum_b, bytes}, {in.accum_sq_b, bytes}, {out_dev, bytes}, {err_dev, bytes / 3u}}))
		return fail(ctx, kInvalid, name + "the sum buffers, out_dev and err_dev must not alias");
	if (any_overlap({{in.feat, fbytes}, {in.feat_sq, fbytes}, {in.accum_a, bytes}, {in.accum_sq_a, bytes}, {in.accum_b, bytes}, {in.accum_sq_b, bytes}, {out_dev, bytes},
	                 {err_dev, bytes / 3u}}))
		return fail(ctx, kInvalid, name + "feat_dev and feat_sq_dev must not alias each other, the sum buffers, out_dev or err_dev");
	if (rmd_status s = levels ? check_levels(ctx, name, *levels) : check_window(ctx, name, radius, patch_radius)) return s;
	if (rmd_status s = check_weights(ctx, name, w.k, w.alpha)) return s;
	if (guided) {
		if (rmd_status s = check_feature_weights(ctx, name, w.k_f, w.tau)) return s;
		if (rmd_status s = check_slope(ctx, name, w.slope)) return s;
	}
	const bool sloped = guided && w.slope > 0.0;
	return rmd::guarded(ctx, what, [&] {
		if (rmd_status s = check_rects(ctx, name, in.rects, in.n_rects, in.W, in.H)) return s;
		if (regional)
			if (rmd_status s = check_rects(ctx, name + "region: ", region, n_region, in.W, in.H)) return s;
		if (rmd_status s = rmd::bind(ctx)) return s;
		std::vector<rmd::DualBlock> table; // the NLM region form's
		rmd::AtrousRegionTables tables;    // the a-trous region form's
		if (regional && !levels) {
			table = rmd::dual_region_table(region, n_region, rmd::denoise_tile_width(radius, patch_radius), rmd::kDenoiseTile);
			if (table.size() > 0x7fffffffu) return fail(ctx, kInvalid, name + "region of more than 2^31 - 1 workgroups");
			if (table.empty()) return finish(ctx); // nothing to write: the call still waits and reports an earlier fault
		} else if (regional) {
			tables = rmd::atrous_region_tables<64, 4>(region, n_region, in.W, in.H, *levels); // (denoise_atrous_dual.hip: kAtrousDualBlockW x kAtrousDualBlockH)
			if (tables.too_large == rmd::AtrousRegionTables::kFrameTooLarge) return fail(ctx, kInvalid, name + "frame of more than 2^31 - 1 workgroups");
			if (tables.too_large) return fail(ctx, kInvalid, name + "region of more than 2^31 - 1 workgroups");
			if (tables.count[*levels] == 0u) return finish(ctx); // nothing to write, as above
		}
		const std::vector<rmd::DualBlock> &blocks = levels ? tables.table : table;
		const rmd::ScratchForm form = !levels ? rmd::kScratchDual : regional ? rmd::kScratchAtrousDualRegion : rmd::kScratchAtrousDual;
		Scratch sc; // (only the a-trous region form keeps its block between calls)
		if (rmd_status s = sc.carve(ctx, rmd::denoise_scratch_layout(form, in.W, in.H, in.n_rects, guided, 0u, blocks.size(), sloped && !levels, sloped && levels),
		                            form == rmd::kScratchAtrousDualRegion ? &ctx->atrous_region_scratch : nullptr))
			return s;
		if (rmd_status s = upload_rects(ctx, sc, in)) return s;
		rmd::DualBlock *d_table = sc.part<rmd::DualBlock>(rmd::kPartTable);
		if (d_table) RMD_HIP(ctx, hipMemcpyAsync(d_table, blocks.data(), blocks.size() * sizeof(rmd::DualBlock), hipMemcpyHostToDevice, ctx->stream));
		uint32_t *n_img = sc.part<uint32_t>(rmd::kPartCountImg), *n_f_img = sc.part<uint32_t>(rmd::kPartFeatCountImg);
		double *planes = sc.part<double>(rmd::kPartPlanes), *feat_planes = sc.part<double>(rmd::kPartFeatPlanes), *slope_planes = sc.part<double>(rmd::kPartSlopePlanes);
		if (!levels)
			RMD_HIP(ctx, rmd::launch_denoise_dual(ctx->stream, in, w, radius, patch_radius, n_img, planes, sc.part<double>(rmd::kPartFb), n_f_img, feat_planes, slope_planes,
			                                      d_table, (uint32_t)table.size(), out_dev, err_dev));
		else if (regional) {
			if (slope_planes && *levels != 0u) ctx->atrous_region_slope_offset = sc.layout.offset[rmd::kPartSlopePlanes], ctx->atrous_region_slope_pixels = (size_t)in.W * in.H;
			RMD_HIP(ctx, rmd::launch_denoise_atrous_dual_region(ctx->stream, in, w, *levels, n_img, planes, n_f_img, feat_planes, slope_planes, d_table, tables.first.data(),
			                                                    tables.count.data(), out_dev, err_dev));
		} else RMD_HIP(ctx, rmd::launch_denoise_atrous_dual(ctx->stream, in, w, *levels, n_img, planes, n_f_img, feat_planes, slope_planes, out_dev, err_dev));
		return finish(ctx);
	});
}

// ---------------------------------------------------------------- the selecting filter (denoise_dual.hip)
// rmd_denoise_dual_select and rmd_denoise_dual_select_slope (denoise_dual.hip): the window is checked before the candidates, aliasing last.  cand_slopes: the
// _slope call's host array (null: every slope 0, and then exactly the launches and the scratch of rmd_denoise_dual_select), read for guided candidates only
rmd_status denoise_dual_select(const char *what, rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev, const double *accum_sq_b_dev,
                                   const double *feat_dev, const double *feat_sq_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                                   const uint32_t *rect_counts_a, const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects, uint32_t radius,
                                   uint32_t patch_radius, const rmd_denoise_candidate *cands, const double *cand_slopes, uint32_t n_cands, uint32_t sure_window,
                                   uint32_t select_window, double *out_dev, double *err_dev, double *sure_dev, uint32_t *win_dev) {
	const std::string name = std::string(what) + ": ";
	DenoiseInput in = dual_input(accum_a_dev, accum_sq_a_dev, accum_b_dev, accum_sq_b_dev, feat_dev, feat_sq_dev, width, height, rects, rect_counts_a, rect_counts_b,
	                                   rect_counts_f, n_rects);
	if (rmd_status s = check_frame(ctx, name, in, true, out_dev)) return s;
	if (!cands || n_cands == 0 || n_cands > rmd::kDenoiseMaxCandidates) return fail(ctx, kInvalid, name + "n_cands must be 1 .. 4, cands not NULL");
	if (sure_window > rmd::kDenoiseMaxSelectWindow || select_window > rmd::kDenoiseMaxSelectWindow) return fail(ctx, kInvalid, name + "sure_window and select_window must be <= 5");
	if (rmd_status s = check_features(ctx, name, in, false)) return s;
	if (rmd_status s = check_window(ctx, name, radius, patch_radius)) return s;
	bool guided = false; // a guided candidate: only then are the features read
	bool sloped = false; // ... with a slope > 0: only then are the slope planes made
	for (uint32_t i = 0; i < n_cands; i++) {
		const rmd_denoise_candidate &c = cands[i];
		const std::string who = name + "candidate " + std::to_string(i) + ": ";
		if (c.reserved != 0u) return fail(ctx, kInvalid, who + "reserved must be 0");
		if (rmd_status s = check_weights(ctx, who, c.k, c.alpha)) return s;
		if (!c.guided) continue;
		guided = true;
		if (!feat_dev) return fail(ctx, kInvalid, who + "guided, but feat_dev and feat_sq_dev are NULL");
		if (n_rects && !rect_counts_f) return fail(ctx, kInvalid, who + "guided, but rect_counts_f is NULL with n_rects > 0");
		if (rmd_status s = check_feature_weights(ctx, who, c.k_f, c.tau)) return s;
		if (cand_slopes) {
			if (rmd_status s = check_slope(ctx, who, cand_slopes[i])) return s;
			sloped = sloped || cand_slopes[i] > 0.0;
		}
	}
	// no two ranges overlap: five of W*H*3 doubles; err_dev's and sure_dev's W*H doubles, win_dev's W*H words, the two of W*H*7 doubles, where given
	const unsigned __int128 n = (unsigned __int128)width * height;
	if (any_overlap({{accum_a_dev, n * 24u}, {accum_sq_a_dev, n * 24u}, {accum_b_dev, n * 24u}, {accum_sq_b_dev, n * 24u}, {out_dev, n * 24u}, {err_dev, n * 8u}, {sure_dev, n * 8u},
	                 {win_dev, n * 4u}, {feat_dev, n * 8u * RMD_FEATURE_CHANNELS}, {feat_sq_dev, n * 8u * RMD_FEATURE_CHANNELS}}))
		return fail(ctx, kInvalid, name + "the sum buffers, the feature buffers, out_dev, err_dev, sure_dev and win_dev must not alias");
	return rmd::guarded(ctx, what, [&] {
		if (rmd_status s = check_rects(ctx, name, rects, n_rects, width, height)) return s;
		if (rmd_status s = rmd::bind(ctx)) return s;
		if (!guided) in.feat = in.feat_sq = nullptr;
		Scratch sc;
		if (rmd_status s = sc.carve(ctx, rmd::denoise_scratch_layout(rmd::kScratchDualSelect, width, height, n_rects, guided, n_cands, 0u, sloped))) return s;
		if (rmd_status s = upload_rects(ctx, sc, in)) return s;
		RMD_HIP(ctx, rmd::launch_denoise_dual_select(ctx->stream, in, radius, patch_radius, cands, sloped ? cand_slopes : nullptr, n_cands, sure_window, select_window,
		                                             sc.part<uint32_t>(rmd::kPartCountImg), sc.part<double>(rmd::kPartPlanes), sc.part<double>(rmd::kPartCand),
		                                             sc.part<double>(rmd::kPartGain), sc.part<uint32_t>(rmd::kPartWinImg), sc.part<uint32_t>(rmd::kPartFeatCountImg),
		                                             sc.part<double>(rmd::kPartFeatPlanes), sc.part<double>(rmd::kPartSlopePlanes), out_dev, err_dev, sure_dev, win_dev));
		return finish(ctx);
	});
}

// ---------------------------------------------------------------- the per-tile measures (tile_luma.hip, tile_weighted.hip)
// rmd_tile_luma_error and rmd_tile_weighted_error.  Their refusals in the header's order, the context last: bad_param() is the rule's own parameter check
// — the refusal's text, or null — in its place in that order; the rects follow rmd_tile_error's rule (inside the frame; they may overlap or repeat), not the
// filters'.  table_host: the call's n_table doubles (luma: none).  The rects, the counts and the table go up in ONE copy from a host block laid out like the
// device's.  keep: the context's block of this measure, kept between calls; launch(in, table_dev, out_dev): the rule's launcher on the uploaded rects
template <class Result, class BadParam, class Launch>
rmd_status tile_measure(const char *what, rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                        const uint32_t *rect_counts, uint32_t n_rects, const double *table_host, uint32_t n_table, Result *out_host, rmd::DeviceBuffer rmd_context::*keep,
                        BadParam bad_param, Launch launch) {
	const std::string name = std::string(what) + ": ";
	return rmd::guarded(ctx, what, [&] {
		if (!accum_dev || !accum_sq_dev || width == 0 || height == 0 || (n_rects && (!rects || !rect_counts || (n_table && !table_host) || !out_host)))
			return fail(ctx, kInvalid, name + "bad argument");
		const unsigned __int128 bytes = (unsigned __int128)width * height * 3u * sizeof(double);
		if (any_overlap({{accum_dev, bytes}, {accum_sq_dev, bytes}})) return fail(ctx, kInvalid, name + "accum_sq_dev must not alias accum_dev");
		if (const char *why = bad_param()) return fail(ctx, kInvalid, name + why);
		if (!rmd::rects_inside(rects, n_rects, width, height)) return fail(ctx, kInvalid, name + rmd::kRectOutside);
		if (rmd_status s = rmd::bind(ctx)) return s;
		std::vector<unsigned char> staged; // (read by the copy until finish() has waited)
		if (n_rects != 0) {
			DenoiseInput in = single_input(accum_dev, accum_sq_dev, nullptr, nullptr, width, height, rects, rect_counts, n_rects);
			size_t upload_bytes = 0;
			Scratch sc; // (the context's block: kept between calls)
			if (rmd_status s = sc.carve(ctx, rmd::tile_measure_scratch_layout(n_rects, sizeof(Result), n_table, &upload_bytes), &(ctx->*keep))) return s;
			staged.assign(upload_bytes, 0);
			std::memcpy(staged.data() + sc.layout.offset[rmd::kPartRects], rects, (size_t)n_rects * sizeof(rmd_tile_rect));
			std::memcpy(staged.data() + sc.layout.offset[rmd::kPartCountsA], rect_counts, (size_t)n_rects * sizeof(uint32_t));
			if (n_table) std::memcpy(staged.data() + sc.layout.offset[rmd::kPartTable], table_host, (size_t)n_table * sizeof(double));
			RMD_HIP(ctx, hipMemcpyAsync(sc.base, staged.data(), upload_bytes, hipMemcpyHostToDevice, ctx->stream));
			in.rects = sc.part<rmd_tile_rect>(rmd::kPartRects), in.counts_a = sc.part<uint32_t>(rmd::kPartCountsA);
			Result *d_out = sc.part<Result>(rmd::kPartTileErrors);
			RMD_HIP(ctx, launch(in, sc.part<double>(rmd::kPartTable), d_out));
			RMD_HIP(ctx, hipMemcpyAsync(out_host, d_out, (size_t)n_rects * sizeof(Result), hipMemcpyDeviceToHost, ctx->stream));
		}
		return finish(ctx); // (n_rects == 0: nothing is launched; the call still waits and reports an earlier fault)
	});
}
// rmd_tile_error and rmd_tile_error_dual behind their checks and the context: the rects go up, launch(rects_dev, out_dev) writes a double per rect
// (kScratchTileError: the rects, then the results), the results come down, the wait
template <class Launch>
rmd_status tile_errors(rmd_context *ctx, uint32_t width, uint32_t height, const rmd_tile_rect *rects, uint32_t n_rects, double *out_err_host, Launch launch) {
	Scratch sc; // (it outlives the wait below)
	if (n_rects != 0) {
		if (rmd_status s = sc.carve(ctx, rmd::denoise_scratch_layout(rmd::kScratchTileError, width, height, n_rects, false, 0u, 0u))) return s;
		rmd_tile_rect *d_rects = sc.part<rmd_tile_rect>(rmd::kPartRects); // (no counts, no count image: not upload_rects's pass over the rects)
		double *d_out = sc.part<double>(rmd::kPartTileErrors);
		RMD_HIP(ctx, hipMemcpyAsync(d_rects, rects, (size_t)n_rects * sizeof(rmd_tile_rect), hipMemcpyHostToDevice, ctx->stream));
		RMD_HIP(ctx, launch(d_rects, d_out));
		RMD_HIP(ctx, hipMemcpyAsync(out_err_host, d_out, (size_t)n_rects * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	}
	return finish(ctx);
}
// A rule header's result struct is the C header's: the same size, and field `f` at the same offset
#define RMD_SAME_FIELD(A, B, f) (sizeof(A) == sizeof(B) && offsetof(A, f) == offsetof(B, f))
} // namespace

extern "C" {

rmd_status rmd_denoise(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                       const uint32_t *rect_sample_counts, uint32_t n_rects, uint32_t radius, uint32_t patch_radius, double k, double alpha,
                       double *out_dev) {
	const DenoiseInput in = single_input(accum_dev, accum_sq_dev, nullptr, nullptr, width, height, rects, rect_sample_counts, n_rects);
	return denoise_single("rmd_denoise", ctx, in, nullptr, radius, patch_radius, {k, alpha, 0.0, 0.0}, out_dev);
}

rmd_status rmd_denoise_guided(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, const double *feat_dev, const double *feat_sq_dev,
                              uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects,
                              uint32_t radius, uint32_t patch_radius, double k, double alpha, double k_f, double tau, double *out_dev) {
	const DenoiseInput in = single_input(accum_dev, accum_sq_dev, feat_dev, feat_sq_dev, width, height, rects, rect_sample_counts, n_rects);
	return denoise_single("rmd_denoise_guided", ctx, in, nullptr, radius, patch_radius, {k, alpha, k_f, tau}, out_dev);
}

rmd_status rmd_denoise_atrous(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, const double *feat_dev, const double *feat_sq_dev,
                              uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects,
                              uint32_t levels, double k, double alpha, double k_f, double tau, double *out_dev) {
	const DenoiseInput in = single_input(accum_dev, accum_sq_dev, feat_dev, feat_sq_dev, width, height, rects, rect_sample_counts, n_rects);
	return denoise_single("rmd_denoise_atrous", ctx, in, &levels, 0u, 0u, {k, alpha, k_f, tau}, out_dev);
}

rmd_status rmd_denoise_dual(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev, const double *accum_sq_b_dev,
                            uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_counts_a, const uint32_t *rect_counts_b,
                            uint32_t n_rects, uint32_t radius, uint32_t patch_radius, double k, double alpha, double *out_dev, double *err_dev) {
	const DenoiseInput in = dual_input(accum_a_dev, accum_sq_a_dev, accum_b_dev, accum_sq_b_dev, nullptr, nullptr, width, height, rects, rect_counts_a, rect_counts_b,
	                                   nullptr, n_rects);
	return denoise_dual("rmd_denoise_dual", false, ctx, in, nullptr, 0u, nullptr, radius, patch_radius, {k, alpha, 0.0, 0.0}, out_dev, err_dev);
}

rmd_status rmd_denoise_dual_region(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev, const double *accum_sq_b_dev,
                                   uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_counts_a, const uint32_t *rect_counts_b,
                                   uint32_t n_rects, const rmd_tile_rect *region, uint32_t n_region, uint32_t radius, uint32_t patch_radius, double k, double alpha,
                                   double *out_dev, double *err_dev) {
	const DenoiseInput in = dual_input(accum_a_dev, accum_sq_a_dev, accum_b_dev, accum_sq_b_dev, nullptr, nullptr, width, height, rects, rect_counts_a, rect_counts_b,
	                                   nullptr, n_rects);
	return denoise_dual("rmd_denoise_dual_region", true, ctx, in, region, n_region, nullptr, radius, patch_radius, {k, alpha, 0.0, 0.0}, out_dev, err_dev);
}

rmd_status rmd_denoise_dual_guided(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev, const double *accum_sq_b_dev,
                                   const double *feat_dev, const double *feat_sq_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                                   const uint32_t *rect_counts_a, const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects, uint32_t radius,
                                   uint32_t patch_radius, double k, double alpha, double k_f, double tau, double *out_dev, double *err_dev) {
	const DenoiseInput in = dual_input(accum_a_dev, accum_sq_a_dev, accum_b_dev, accum_sq_b_dev, feat_dev, feat_sq_dev, width, height, rects, rect_counts_a, rect_counts_b,
	                                   rect_counts_f, n_rects);
	return denoise_dual("rmd_denoise_dual_guided", false, ctx, in, nullptr, 0u, nullptr, radius, patch_radius, {k, alpha, k_f, tau}, out_dev, err_dev);
}

rmd_status rmd_denoise_dual_guided_region(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev,
                                          const double *accum_sq_b_dev, const double *feat_dev, const double *feat_sq_dev, uint32_t width, uint32_t height,
                                          const rmd_tile_rect *rects, const uint32_t *rect_counts_a, const uint32_t *rect_counts_b, const uint32_t *rect_counts_f,
                                          uint32_t n_rects, const rmd_tile_rect *region, uint32_t n_region, uint32_t radius, uint32_t patch_radius, double k,
                                          double alpha, double k_f, double tau, double *out_dev, double *err_dev) {
	const DenoiseInput in = dual_input(accum_a_dev, accum_sq_a_dev, accum_b_dev, accum_sq_b_dev, feat_dev, feat_sq_dev, width, height, rects, rect_counts_a, rect_counts_b,
	                                   rect_counts_f, n_rects);
	return denoise_dual("rmd_denoise_dual_guided_region", true, ctx, in, region, n_region, nullptr, radius, patch_radius, {k, alpha, k_f, tau}, out_dev, err_dev);
}

rmd_status rmd_denoise_atrous_dual(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev, const double *accum_sq_b_dev,
                                   const double *feat_dev, const double *feat_sq_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                                   const uint32_t *rect_counts_a, const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects, uint32_t levels,
                                   double k, double alpha, double k_f, double tau, double *out_dev, double *err_dev) {
	const DenoiseInput in = dual_input(accum_a_dev, accum_sq_a_dev, accum_b_dev, accum_sq_b_dev, feat_dev, feat_sq_dev, width, height, rects, rect_counts_a, rect_counts_b,
	                                   rect_counts_f, n_rects);
	return denoise_dual("rmd_denoise_atrous_dual", false, ctx, in, nullptr, 0u, &levels, 0u, 0u, {k, alpha, k_f, tau}, out_dev, err_dev);
}

rmd_status rmd_denoise_atrous_dual_region(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev,
                                          const double *accum_sq_b_dev, const double *feat_dev, const double *feat_sq_dev, uint32_t width, uint32_t height,
                                          const rmd_tile_rect *rects, const uint32_t *rect_counts_a, const uint32_t *rect_counts_b, const uint32_t *rect_counts_f,
                                          uint32_t n_rects, const rmd_tile_rect *region, uint32_t n_region, uint32_t levels, double k, double alpha, double k_f,
                                          double tau, double *out_dev, double *err_dev) {
	const DenoiseInput in = dual_input(accum_a_dev, accum_sq_a_dev, accum_b_dev, accum_sq_b_dev, feat_dev, feat_sq_dev, width, height, rects, rect_counts_a, rect_counts_b,
	                                   rect_counts_f, n_rects);
	return denoise_dual("rmd_denoise_atrous_dual_region", true, ctx, in, region, n_region, &levels, 0u, 0u, {k, alpha, k_f, tau}, out_dev, err_dev);
}

rmd_status rmd_denoise_dual_select(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev, const double *accum_sq_b_dev,
                                   const double *feat_dev, const double *feat_sq_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                                   const uint32_t *rect_counts_a, const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects, uint32_t radius,
                                   uint32_t patch_radius, const rmd_denoise_candidate *cands, uint32_t n_cands, uint32_t sure_window, uint32_t select_window,
                                   double *out_dev, double *err_dev, double *sure_dev, uint32_t *win_dev) {
	return denoise_dual_select("rmd_denoise_dual_select", ctx, accum_a_dev, accum_sq_a_dev, accum_b_dev, accum_sq_b_dev, feat_dev, feat_sq_dev, width, height, rects,
	                           rect_counts_a, rect_counts_b, rect_counts_f, n_rects, radius, patch_radius, cands, nullptr, n_cands, sure_window, select_window, out_dev, err_dev,
	                           sure_dev, win_dev);
}

rmd_status rmd_denoise_dual_select_slope(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev,
                                         const double *accum_sq_b_dev, const double *feat_dev, const double *feat_sq_dev, uint32_t width, uint32_t height,
                                         const rmd_tile_rect *rects, const uint32_t *rect_counts_a, const uint32_t *rect_counts_b, const uint32_t *rect_counts_f,
                                         uint32_t n_rects, uint32_t radius, uint32_t patch_radius, const rmd_denoise_candidate *cands, const double *cand_slopes,
                                         uint32_t n_cands, uint32_t sure_window, uint32_t select_window, double *out_dev, double *err_dev, double *sure_dev,
                                         uint32_t *win_dev) {
	return denoise_dual_select("rmd_denoise_dual_select_slope", ctx, accum_a_dev, accum_sq_a_dev, accum_b_dev, accum_sq_b_dev, feat_dev, feat_sq_dev, width, height, rects,
	                           rect_counts_a, rect_counts_b, rect_counts_f, n_rects, radius, patch_radius, cands, cand_slopes, n_cands, sure_window, select_window, out_dev,
	                           err_dev, sure_dev, win_dev);
}

rmd_status rmd_denoise_guided_slope(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, const double *feat_dev, const double *feat_sq_dev,
                                    uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects,
                                    uint32_t radius, uint32_t patch_radius, double k, double alpha, double k_f, double tau, double slope, double *out_dev) {
	const DenoiseInput in = single_input(accum_dev, accum_sq_dev, feat_dev, feat_sq_dev, width, height, rects, rect_sample_counts, n_rects);
	return denoise_single("rmd_denoise_guided_slope", ctx, in, nullptr, radius, patch_radius, {k, alpha, k_f, tau, slope}, out_dev);
}

rmd_status rmd_denoise_dual_guided_slope(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev,
                                         const double *accum_sq_b_dev, const double *feat_dev, const double *feat_sq_dev, uint32_t width, uint32_t height,
                                         const rmd_tile_rect *rects, const uint32_t *rect_counts_a, const uint32_t *rect_counts_b, const uint32_t *rect_counts_f,
                                         uint32_t n_rects, uint32_t radius, uint32_t patch_radius, double k, double alpha, double k_f, double tau, double slope,
                                         double *out_dev, double *err_dev) {
	const DenoiseInput in = dual_input(accum_a_dev, accum_sq_a_dev, accum_b_dev, accum_sq_b_dev, feat_dev, feat_sq_dev, width, height, rects, rect_counts_a, rect_counts_b,
	                                   rect_counts_f, n_rects);
	return denoise_dual("rmd_denoise_dual_guided_slope", false, ctx, in, nullptr, 0u, nullptr, radius, patch_radius, {k, alpha, k_f, tau, slope}, out_dev, err_dev);
}

rmd_status rmd_denoise_dual_guided_slope_region(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev,
                                                const double *accum_sq_b_dev, const double *feat_dev, const double *feat_sq_dev, uint32_t width, uint32_t height,
                                                const rmd_tile_rect *rects, const uint32_t *rect_counts_a, const uint32_t *rect_counts_b,
                                                const uint32_t *rect_counts_f, uint32_t n_rects, const rmd_tile_rect *region, uint32_t n_region, uint32_t radius,
                                                uint32_t patch_radius, double k, double alpha, double k_f, double tau, double slope, double *out_dev, double *err_dev) {
	const DenoiseInput in = dual_input(accum_a_dev, accum_sq_a_dev, accum_b_dev, accum_sq_b_dev, feat_dev, feat_sq_dev, width, height, rects, rect_counts_a, rect_counts_b,
	                                   rect_counts_f, n_rects);
	return denoise_dual("rmd_denoise_dual_guided_slope_region", true, ctx, in, region, n_region, nullptr, radius, patch_radius, {k, alpha, k_f, tau, slope}, out_dev, err_dev);
}

rmd_status rmd_denoise_atrous_slope(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, const double *feat_dev, const double *feat_sq_dev,
                                    uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects,
                                    uint32_t levels, double k, double alpha, double k_f, double tau, double slope, double *out_dev) {
	const DenoiseInput in = single_input(accum_dev, accum_sq_dev, feat_dev, feat_sq_dev, width, height, rects, rect_sample_counts, n_rects);
	return denoise_single("rmd_denoise_atrous_slope", ctx, in, &levels, 0u, 0u, {k, alpha, k_f, tau, slope}, out_dev);
}

rmd_status rmd_denoise_atrous_dual_slope(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev,
                                         const double *accum_sq_b_dev, const double *feat_dev, const double *feat_sq_dev, uint32_t width, uint32_t height,
                                         const rmd_tile_rect *rects, const uint32_t *rect_counts_a, const uint32_t *rect_counts_b, const uint32_t *rect_counts_f,
                                         uint32_t n_rects, uint32_t levels, double k, double alpha, double k_f, double tau, double slope, double *out_dev,
                                         double *err_dev) {
	const DenoiseInput in = dual_input(accum_a_dev, accum_sq_a_dev, accum_b_dev, accum_sq_b_dev, feat_dev, feat_sq_dev, width, height, rects, rect_counts_a, rect_counts_b,
	                                   rect_counts_f, n_rects);
	return denoise_dual("rmd_denoise_atrous_dual_slope", false, ctx, in, nullptr, 0u, &levels, 0u, 0u, {k, alpha, k_f, tau, slope}, out_dev, err_dev);
}

rmd_status rmd_denoise_atrous_dual_slope_region(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev,
                                                const double *accum_sq_b_dev, const double *feat_dev, const double *feat_sq_dev, uint32_t width, uint32_t height,
                                                const rmd_tile_rect *rects, const uint32_t *rect_counts_a, const uint32_t *rect_counts_b,
                                                const uint32_t *rect_counts_f, uint32_t n_rects, const rmd_tile_rect *region, uint32_t n_region, uint32_t levels,
                                                double k, double alpha, double k_f, double tau, double slope, double *out_dev, double *err_dev) {
	const DenoiseInput in = dual_input(accum_a_dev, accum_sq_a_dev, accum_b_dev, accum_sq_b_dev, feat_dev, feat_sq_dev, width, height, rects, rect_counts_a, rect_counts_b,
	                                   rect_counts_f, n_rects);
	return denoise_dual("rmd_denoise_atrous_dual_slope_region", true, ctx, in, region, n_region, &levels, 0u, 0u, {k, alpha, k_f, tau, slope}, out_dev, err_dev);
}

// rmd_despike (despike.hip).  Its refusals in the header's order: the frame and the rects first, the buffers after the parameters, the context last
rmd_status rmd_despike(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                       const uint32_t *rect_sample_counts, uint32_t n_rects, uint32_t radius, uint32_t rank, double k, double ratio, double floor,
                       double *out_accum_dev, double *out_accum_sq_dev, uint32_t *replaced_host) {
	const std::string name = "rmd_despike: ";
	return rmd::guarded(ctx, "rmd_despike", [&] {
		if (width == 0 || height == 0 || (n_rects && (!rects || !rect_sample_counts))) return fail(ctx, kInvalid, name + "bad argument");
		if (rmd_status s = check_rects(ctx, name, rects, n_rects, width, height)) return s;
		if (radius < 1u || radius > rmd::kDespikeMaxRadius) return fail(ctx, kInvalid, name + "radius must be 1 .. 3");
		if (rank > (2u * radius + 1u) * (2u * radius + 1u) - 2u) return fail(ctx, kInvalid, name + "rank must be <= (2 * radius + 1)^2 - 2");
		if (!(k >= 0.0) || !std::isfinite(k)) return fail(ctx, kInvalid, name + "k must be finite and >= 0");
		if (!(ratio >= 1.0) || !std::isfinite(ratio)) return fail(ctx, kInvalid, name + "ratio must be finite and >= 1");
		if (!(floor >= 0.0) || !std::isfinite(floor)) return fail(ctx, kInvalid, name + "floor must be finite and >= 0");
		if (!accum_dev || !accum_sq_dev || !out_accum_dev || !out_accum_sq_dev) return fail(ctx, kInvalid, name + "the four sum buffers must not be NULL");
		const unsigned __int128 bytes = (unsigned __int128)width * height * 3u * sizeof(double);
		if (any_overlap({{accum_dev, bytes}, {accum_sq_dev, bytes}, {out_accum_dev, bytes}, {out_accum_sq_dev, bytes}}))
			return fail(ctx, kInvalid, name + "accum_dev, accum_sq_dev, out_accum_dev and out_accum_sq_dev must not alias");
		if (rmd_status s = rmd::bind(ctx)) return s;
		DenoiseInput in = single_input(accum_dev, accum_sq_dev, nullptr, nullptr, width, height, rects, rect_sample_counts, n_rects);
		Scratch sc; // (the context's block: kept between calls)
		if (rmd_status s = sc.carve(ctx, rmd::despike_scratch_layout(width, height, n_rects), &ctx->despike_scratch)) return s;
		if (rmd_status s = upload_rects(ctx, sc, in)) return s;
		uint32_t *d_replaced = replaced_host && n_rects ? sc.part<uint32_t>(rmd::kPartTileErrors) : nullptr;
		RMD_HIP(ctx, rmd::launch_despike(ctx->stream, in, radius, rank, k, ratio, floor, sc.part<uint32_t>(rmd::kPartCountImg), sc.part<uint32_t>(rmd::kPartWinImg),
		                                 out_accum_dev, out_accum_sq_dev, d_replaced));
		if (d_replaced) RMD_HIP(ctx, hipMemcpyAsync(replaced_host, d_replaced, (size_t)n_rects * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		return finish(ctx);
	});
}

// rmd_despike_dual (despike_dual.hip).  rmd_despike's refusals in its order and texts, with the counts' sum after the rects and eight buffers in place of four
rmd_status rmd_despike_dual(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev, const double *accum_sq_b_dev,
                            uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_counts_a, const uint32_t *rect_counts_b, uint32_t n_rects,
                            uint32_t radius, uint32_t rank, double k, double ratio, double floor, double *out_accum_a_dev, double *out_accum_sq_a_dev,
                            double *out_accum_b_dev, double *out_accum_sq_b_dev, uint32_t *replaced_host) {
	const std::string name = "rmd_despike_dual: ";
	return rmd::guarded(ctx, "rmd_despike_dual", [&] {
		if (width == 0 || height == 0 || (n_rects && (!rects || !rect_counts_a || !rect_counts_b))) return fail(ctx, kInvalid, name + "bad argument");
		if (rmd_status s = check_rects(ctx, name, rects, n_rects, width, height)) return s;
		for (uint32_t j = 0; j < n_rects; j++)
			if ((uint64_t)rect_counts_a[j] + rect_counts_b[j] > 0xFFFFFFFFull) return fail(ctx, kInvalid, name + "a rect's two counts must not add to more than 2^32 - 1");
		if (radius < 1u || radius > rmd::kDespikeMaxRadius) return fail(ctx, kInvalid, name + "radius must be 1 .. 3");
		if (rank > (2u * radius + 1u) * (2u * radius + 1u) - 2u) return fail(ctx, kInvalid, name + "rank must be <= (2 * radius + 1)^2 - 2");
		if (!(k >= 0.0) || !std::isfinite(k)) return fail(ctx, kInvalid, name + "k must be finite and >= 0");
		if (!(ratio >= 1.0) || !std::isfinite(ratio)) return fail(ctx, kInvalid, name + "ratio must be finite and >= 1");
		if (!(floor >= 0.0) || !std::isfinite(floor)) return fail(ctx, kInvalid, name + "floor must be finite and >= 0");
		if (!accum_a_dev || !accum_sq_a_dev || !accum_b_dev || !accum_sq_b_dev || !out_accum_a_dev || !out_accum_sq_a_dev || !out_accum_b_dev || !out_accum_sq_b_dev)
			return fail(ctx, kInvalid, name + "the eight sum buffers must not be NULL");
		const unsigned __int128 bytes = (unsigned __int128)width * height * 3u * sizeof(double);
		if (any_overlap({{accum_a_dev, bytes}, {accum_sq_a_dev, bytes}, {accum_b_dev, bytes}, {accum_sq_b_dev, bytes}, {out_accum_a_dev, bytes}, {out_accum_sq_a_dev, bytes},
		                 {out_accum_b_dev, bytes}, {out_accum_sq_b_dev, bytes}}))
			return fail(ctx, kInvalid, name + "the four input and the four output sum buffers must not alias");
		if (rmd_status s = rmd::bind(ctx)) return s;
		DenoiseInput in = dual_input(accum_a_dev, accum_sq_a_dev, accum_b_dev, accum_sq_b_dev, nullptr, nullptr, width, height, rects, rect_counts_a, rect_counts_b, nullptr, n_rects);
		Scratch sc; // (the context's block: kept between calls)
		if (rmd_status s = sc.carve(ctx, rmd::despike_dual_scratch_layout(width, height, n_rects), &ctx->despike_dual_scratch)) return s;
		if (rmd_status s = upload_rects(ctx, sc, in)) return s;
		uint32_t *d_replaced = replaced_host && n_rects ? sc.part<uint32_t>(rmd::kPartTileErrors) : nullptr;
		RMD_HIP(ctx, rmd::launch_despike_dual(ctx->stream, in, radius, rank, k, ratio, floor, sc.part<uint32_t>(rmd::kPartCountImg), sc.part<uint32_t>(rmd::kPartWinImg),
		                                      out_accum_a_dev, out_accum_sq_a_dev, out_accum_b_dev, out_accum_sq_b_dev, d_replaced));
		if (d_replaced) RMD_HIP(ctx, hipMemcpyAsync(replaced_host, d_replaced, (size_t)n_rects * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		return finish(ctx);
	});
}

rmd_status rmd_tile_luma_error(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                               const uint32_t *rect_counts, uint32_t n_rects, double floor, rmd_tile_luma *out_host) {
	using A = rmd::TileLuma;
	using B = rmd_tile_luma;
	static_assert(RMD_SAME_FIELD(A, B, tile_rms) && RMD_SAME_FIELD(A, B, pixel_rms) && RMD_SAME_FIELD(A, B, mean_luma) && RMD_SAME_FIELD(A, B, mean_variance) &&
	                  RMD_SAME_FIELD(A, B, mean_rel_variance) && RMD_SAME_FIELD(A, B, valid) && RMD_SAME_FIELD(A, B, invalid),
	              "tile_luma_rule.hpp's TileLuma is rmd_tile_luma");
	return tile_measure(
	    "rmd_tile_luma_error", ctx, accum_dev, accum_sq_dev, width, height, rects, rect_counts, n_rects, nullptr, 0u, out_host, &rmd_context::tile_luma_scratch,
	    [&]() -> const char * { return !(floor > 0.0) || !std::isfinite(floor) ? "floor must be finite and > 0" : nullptr; },
	    [&](const DenoiseInput &in, const double *, B *d_out) { return rmd::launch_tile_luma(ctx->stream, in, floor, reinterpret_cast<A *>(d_out)); });
}

rmd_status rmd_tile_weighted_error(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                                   const uint32_t *rect_counts, uint32_t n_rects, const double *weights_host, rmd_tile_weighted *out_host) {
	using A = rmd::TileWeighted;
	using B = rmd_tile_weighted;
	static_assert(sizeof(B) == 40 && RMD_SAME_FIELD(A, B, rms) && RMD_SAME_FIELD(A, B, mean_weighted_variance) && RMD_SAME_FIELD(A, B, mean_luma) &&
	                  RMD_SAME_FIELD(A, B, mean_variance) && RMD_SAME_FIELD(A, B, valid) && RMD_SAME_FIELD(A, B, invalid),
	              "tile_weighted_rule.hpp's TileWeighted is rmd_tile_weighted");
	static_assert(rmd::kLumaWeights == RMD_LUMA_WEIGHTS, "tile_weighted_rule.hpp's table is the header's");
	return tile_measure(
	    "rmd_tile_weighted_error", ctx, accum_dev, accum_sq_dev, width, height, rects, rect_counts, n_rects, weights_host, RMD_LUMA_WEIGHTS, out_host,
	    &rmd_context::tile_weighted_scratch,
	    [&]() -> const char * {
		    for (uint32_t k = 0; weights_host && k < RMD_LUMA_WEIGHTS; k++)
			    if (!(weights_host[k] >= 0.0) || !std::isfinite(weights_host[k])) return "every weight must be finite and >= 0";
		    return nullptr;
	    },
	    [&](const DenoiseInput &in, const double *weights, B *d_out) { return rmd::launch_tile_weighted(ctx->stream, in, weights, reinterpret_cast<A *>(d_out)); });
}

// The filtered frame's measure: no counts, and the two ranges differ in size, so it is not tile_measure's body; the same order of refusals, the same staged upload
rmd_status rmd_tile_weighted_error_dual(rmd_context *ctx, const double *out_dev, const double *err_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                                        uint32_t n_rects, const double *weights_host, rmd_tile_weighted *out_host) {
	using A = rmd::TileWeighted;
	using B = rmd_tile_weighted;
	const std::string name = "rmd_tile_weighted_error_dual: ";
	return rmd::guarded(ctx, "rmd_tile_weighted_error_dual", [&] {
		if (!out_dev || !err_dev || width == 0 || height == 0 || (n_rects && (!rects || !weights_host || !out_host))) return fail(ctx, kInvalid, name + "bad argument");
		const unsigned __int128 bytes = (unsigned __int128)width * height * sizeof(double);
		if (any_overlap({{out_dev, bytes * 3u}, {err_dev, bytes}})) return fail(ctx, kInvalid, name + "err_dev must not alias out_dev");
		for (uint32_t k = 0; weights_host && k < RMD_LUMA_WEIGHTS; k++)
			if (!(weights_host[k] >= 0.0) || !std::isfinite(weights_host[k])) return fail(ctx, kInvalid, name + "every weight must be finite and >= 0");
		if (!rmd::rects_inside(rects, n_rects, width, height)) return fail(ctx, kInvalid, name + rmd::kRectOutside);
		if (rmd_status s = rmd::bind(ctx)) return s;
		std::vector<unsigned char> staged; // (read by the copy until finish() has waited)
		if (n_rects != 0) {
			size_t upload_bytes = 0;
			Scratch sc; // (the context's block: kept between calls)
			if (rmd_status s = sc.carve(ctx, rmd::tile_weighted_dual_scratch_layout(n_rects, sizeof(B), RMD_LUMA_WEIGHTS, &upload_bytes), &ctx->tile_weighted_dual_scratch)) return s;
			staged.assign(upload_bytes, 0);
			std::memcpy(staged.data() + sc.layout.offset[rmd::kPartRects], rects, (size_t)n_rects * sizeof(rmd_tile_rect));
			std::memcpy(staged.data() + sc.layout.offset[rmd::kPartTable], weights_host, (size_t)RMD_LUMA_WEIGHTS * sizeof(double));
			RMD_HIP(ctx, hipMemcpyAsync(sc.base, staged.data(), upload_bytes, hipMemcpyHostToDevice, ctx->stream));
			B *d_out = sc.part<B>(rmd::kPartTileErrors);
			RMD_HIP(ctx, rmd::launch_tile_weighted_dual(ctx->stream, out_dev, err_dev, sc.part<rmd_tile_rect>(rmd::kPartRects), n_rects, width, sc.part<double>(rmd::kPartTable),
			                                            reinterpret_cast<A *>(d_out)));
			RMD_HIP(ctx, hipMemcpyAsync(out_host, d_out, (size_t)n_rects * sizeof(B), hipMemcpyDeviceToHost, ctx->stream));
		}
		return finish(ctx); // (n_rects == 0: nothing is launched; the call still waits and reports an earlier fault)
	});
}

// The raw frame's measure (kernels.hip: tile_error_kernel).  The context comes before the rects here
rmd_status rmd_tile_error(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height, uint32_t sample_count,
                          double floor, const rmd_tile_rect *rects, uint32_t n_rects, double *out_err_host) {
	if (!accum_dev || !accum_sq_dev || width == 0 || height == 0 || (n_rects && (!rects || !out_err_host))) return fail(ctx, kInvalid, "rmd_tile_error: bad argument");
	if (accum_sq_dev == accum_dev) return fail(ctx, kInvalid, "rmd_tile_error: accum_sq_dev must not alias accum_dev");
	if (!(floor > 0.0) || !std::isfinite(floor)) return fail(ctx, kInvalid, "rmd_tile_error: floor must be finite and > 0");
	return rmd::guarded(ctx, "rmd_tile_error", [&] {
		if (rmd_status s = rmd::bind(ctx)) return s;
		if (!rmd::rects_inside(rects, n_rects, width, height)) return fail(ctx, kInvalid, std::string("rmd_tile_error: ") + rmd::kRectOutside);
		return tile_errors(ctx, width, height, rects, n_rects, out_err_host, [&](const rmd_tile_rect *d_rects, double *d_out) {
			return rmd::launch_tile_error(ctx->stream, accum_dev, accum_sq_dev, d_rects, n_rects, width, sample_count, floor, d_out);
		});
	});
}

rmd_status rmd_tile_error_dual(rmd_context *ctx, const double *err_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects, uint32_t n_rects,
                               double *out_err_host) {
	if (!err_dev || width == 0 || height == 0 || (n_rects && (!rects || !out_err_host))) return fail(ctx, kInvalid, "rmd_tile_error_dual: bad argument");
	if (!rmd::rects_inside(rects, n_rects, width, height)) return fail(ctx, kInvalid, std::string("rmd_tile_error_dual: ") + rmd::kRectOutside);
	return rmd::guarded(ctx, "rmd_tile_error_dual", [&] {
		if (rmd_status s = rmd::bind(ctx)) return s;
		return tile_errors(ctx, width, height, rects, n_rects, out_err_host,
		                   [&](const rmd_tile_rect *d_rects, double *d_out) { return rmd::launch_tile_error_dual(ctx->stream, err_dev, d_rects, n_rects, width, d_out); });
	});
}

} // extern "C"
