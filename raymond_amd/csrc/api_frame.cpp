// C-ABI implementation (include/raymond_hip.h) of what is done with a frame: the framebuffer helpers, the tile transfers, the resolve/tone-map epilogue
// over a frame and over tile rectangles, the luminance histogram, and the host-only exposure and display weights.  Host code only; the kernels are in
// kernels.hip, resolve_tiles.hip and luma_histogram.hip.
#define RMD_WITH_HIP 1
#include <cstddef>

#include "internal.hpp"
#include "launch.hpp"
#include "luma_bins.hpp"
#include "resolve_tiles_host.hpp"
#include "tonemap_host.hpp"

using rmd::bind;

namespace {
// A zeroed width x height buffer of `channels` doubles a pixel, handed to the caller (`bad`: what a bad argument is answered with)
rmd_status alloc_zeroed(rmd_context *ctx, const char *bad, uint32_t width, uint32_t height, size_t channels, double **out_dev) {
	if (rmd_status s = bind(ctx)) return s;
	if (!out_dev || width == 0 || height == 0) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, bad);
	const size_t bytes = (size_t)width * height * channels * sizeof(double);
	RMD_HIP(ctx, hipMalloc((void **)out_dev, bytes));
	RMD_HIP(ctx, hipMemsetAsync(*out_dev, 0, bytes, ctx->stream));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return RMD_OK;
}

// ---------------------------------------------------------------- tile rectangles <-> packed host buffers
rmd_status wait_slot(rmd_context *ctx, rmd_context::TransferSlot &sl) {
	if (sl.in_flight) RMD_HIP(ctx, hipEventSynchronize(sl.copied));
	sl.in_flight = false;
	return RMD_OK;
}
// What both tile transfers start with.  slot stays null when there are no rects: nothing to do, and no slot is taken
struct Transfer {
	rmd_context::TransferSlot *slot = nullptr;
	const rmd_tile_rect *d_rects = nullptr; // the slot's table on the device: the rects ...
	const uint64_t *d_first = nullptr;      // ... and each rect's first packed pixel, of n_pixels in all
	uint64_t n_pixels = 0;
};
// Binds, checks the arguments (`what`: the entry point's name), takes the next slot and waits for it — a third transfer waits for the first — and only
// then looks at the rects: builds the table {rect, first pixel}, makes the slot's device buffers large enough and enqueues the table's upload
rmd_status begin_transfer(rmd_context *ctx, const char *what, const double *dev, const double *host_packed, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                          uint32_t n_rects, Transfer &t) {
	if (rmd_status s = bind(ctx)) return s;
	if (!dev || !host_packed || (n_rects && !rects) || width == 0 || height == 0) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string(what) + ": bad argument");
	if (n_rects == 0) return RMD_OK;
	rmd_context::TransferSlot &sl = ctx->transfer[ctx->next_transfer];
	ctx->next_transfer ^= 1u;
	if (rmd_status s = wait_slot(ctx, sl)) return s;
	std::vector<uint64_t> first;
	if (!rmd::resolve_first_pixels(rects, n_rects, width, height, first)) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, std::string("tile transfer: ") + rmd::kRectOutside);
	const size_t rect_bytes = (size_t)n_rects * sizeof(rmd_tile_rect);
	sl.h_table.resize(rect_bytes + (size_t)n_rects * sizeof(uint64_t));
	std::memcpy(sl.h_table.data(), rects, rect_bytes);
	std::memcpy(sl.h_table.data() + rect_bytes, first.data(), (size_t)n_rects * sizeof(uint64_t));
	RMD_HIP(ctx, sl.packed.grow((size_t)first[n_rects] * 3 * sizeof(double)));
	RMD_HIP(ctx, sl.table.grow(sl.h_table.size()));
	if (!sl.packed_ready) RMD_HIP(ctx, hipEventCreateWithFlags(&sl.packed_ready, hipEventDisableTiming));
	if (!sl.copied) RMD_HIP(ctx, hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming));
	if (!ctx->copy_stream) RMD_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
	RMD_HIP(ctx, hipMemcpyAsync(sl.table.as<void>(), sl.h_table.data(), sl.h_table.size(), hipMemcpyHostToDevice, ctx->stream));
	t.slot = &sl, t.d_rects = sl.table.as<rmd_tile_rect>(), t.n_pixels = first[n_rects];
	t.d_first = reinterpret_cast<const uint64_t *>(sl.table.as<unsigned char>() + rect_bytes);
	return RMD_OK;
}

// ---------------------------------------------------------------- the tone-map calls' end and fix-up
// Where a flagged entry of the kernel's list lies: its sums in the frame (an index in doubles), its three bytes in the output, its sample count
struct FlaggedPixel {
	size_t frame, out;
	double samples;
};
// What both tone-map calls end with, their kernel enqueued: the bytes at `d` (out_bytes of them) and the flag count come down, the stream is waited
// for, and the pixels the kernel flagged — those whose byte an ulp of exp / pow could decide, the count's entries at d_list — are recomputed with the
// host libm, as the reference does every pixel (tonemap_host.hpp).  Many (a synthetic frame): one download of the sums instead of a copy per pixel.
// accum2_dev: the second sum buffer, or null.  locate(entry) -> FlaggedPixel
template <class Locate>
rmd_status finish_tonemap(rmd_context *ctx, const uint8_t *d, size_t out_bytes, const uint32_t *d_count, const uint32_t *d_list, const double *accum_dev,
                          const double *accum2_dev, size_t frame_doubles, double exposure, double inv_gamma, uint8_t *out, Locate locate) {
	uint32_t n_flagged = 0;
	RMD_HIP(ctx, hipMemcpyAsync(out, d, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
	RMD_HIP(ctx, hipMemcpyAsync(&n_flagged, d_count, 4, hipMemcpyDeviceToHost, ctx->stream));
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	std::vector<uint32_t> list(n_flagged);
	if (n_flagged != 0) RMD_HIP(ctx, hipMemcpy(list.data(), d_list, (size_t)n_flagged * 4, hipMemcpyDeviceToHost));
	const bool whole = n_flagged > 1024u;
	std::vector<double> px, px2;
	if (whole) {
		px.resize(frame_doubles);
		RMD_HIP(ctx, hipMemcpy(px.data(), accum_dev, frame_doubles * sizeof(double), hipMemcpyDeviceToHost));
		if (accum2_dev) {
			px2.resize(frame_doubles);
			RMD_HIP(ctx, hipMemcpy(px2.data(), accum2_dev, frame_doubles * sizeof(double), hipMemcpyDeviceToHost));
		}
	}
	for (uint32_t k = 0; k < n_flagged; k++) {
		const FlaggedPixel at = locate(list[k]);
		double a[3], b[3] = {0.0, 0.0, 0.0};
		if (whole) {
			std::memcpy(a, &px[at.frame], sizeof(a));
			if (accum2_dev) std::memcpy(b, &px2[at.frame], sizeof(b));
		} else {
			RMD_HIP(ctx, hipMemcpy(a, accum_dev + at.frame, sizeof(a), hipMemcpyDeviceToHost));
			if (accum2_dev) RMD_HIP(ctx, hipMemcpy(b, accum2_dev + at.frame, sizeof(b), hipMemcpyDeviceToHost));
		}
		if (accum2_dev)
			for (int c = 0; c < 3; c++) a[c] = a[c] + b[c];
		rmd::tonemap_bytes(a, at.samples, exposure, inv_gamma, out + at.out);
	}
	// the frame came from launches this call has waited for: one that was cut short by a device fault is not handed out as an image
	return rmd::check_fault(ctx);
}

// ---------------------------------------------------------------- run tables (resolve_tiles_host.hpp)
// What rmd_resolve_tonemap_tiles and rmd_luminance_histogram_tiles share.  Their argument rules in their shared order (`name`: the call's name and
// ": "), up to the packed pixel count: first[n_rects].  Each call places its context and its null-output rule around this itself
rmd_status check_run_args(rmd_context *ctx, const std::string &name, const double *accum_dev, const double *accum2_dev, uint32_t width, uint32_t height,
                          const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects, std::vector<uint64_t> &first) {
	if (!accum_dev || width == 0 || height == 0 || (n_rects && (!rects || !rect_sample_counts))) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + "bad argument");
	const unsigned __int128 frame_bytes = (unsigned __int128)width * height * 3u * sizeof(double);
	if (rmd::any_overlap({{accum_dev, frame_bytes}, {accum2_dev, frame_bytes}})) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + "accum2_dev overlaps accum_dev");
	if (!rmd::resolve_first_pixels(rects, n_rects, width, height, first)) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + rmd::kRectOutside);
	if (first[n_rects] > 0xFFFFFFFFull) return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, name + "more than 2^32-1 packed pixels");
	return RMD_OK;
}
// ... and, for rects that hold pixels, the table and its way to the device: `keep`'s block grown to [head_bytes][runs], the table's host copy kept
// beside it and its upload enqueued.  The stream is waited for before anything is enqueued (the call waits for the frame's renders in any case): the
// table's upload and the call's downloads, which may go to pageable memory, are then made on an idle stream, as rmd_resolve_tonemap's are by every
// caller here.  head_bytes: a multiple of 16
rmd_status upload_run_table(rmd_context *ctx, const std::string &name, const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects,
                            const std::vector<uint64_t> &first, rmd_context::RunTable &keep, size_t head_bytes, rmd::ResolveRun **d_runs, uint32_t *n_runs) {
	const std::vector<rmd::ResolveRun> runs = rmd::resolve_runs(rects, rect_sample_counts, n_rects, first);
	if (runs.size() > 0x7FFFFFFFull) return rmd::fail(ctx, RMD_ERR_UNSUPPORTED, name + "more than 2^31-1 workgroups");
	const size_t table_bytes = runs.size() * sizeof(rmd::ResolveRun);
	RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
	RMD_HIP(ctx, keep.block.grow(head_bytes + table_bytes));
	keep.host.assign(reinterpret_cast<const unsigned char *>(runs.data()), reinterpret_cast<const unsigned char *>(runs.data()) + table_bytes);
	*d_runs = reinterpret_cast<rmd::ResolveRun *>(keep.block.as<unsigned char>() + head_bytes), *n_runs = (uint32_t)runs.size();
	RMD_HIP(ctx, hipMemcpyAsync(*d_runs, keep.host.data(), table_bytes, hipMemcpyHostToDevice, ctx->stream));
	return RMD_OK;
}
} // namespace

extern "C" {

rmd_status rmd_framebuffer_alloc(rmd_context *ctx, uint32_t width, uint32_t height, double **out_dev) {
	return alloc_zeroed(ctx, "rmd_framebuffer_alloc: bad argument", width, height, 3, out_dev);
}
// first-hit feature buffers (features.hip)
rmd_status rmd_feature_buffer_alloc(rmd_context *ctx, uint32_t width, uint32_t height, double **out_dev) {
	return alloc_zeroed(ctx, "rmd_feature_buffer_alloc: bad argument", width, height, RMD_FEATURE_CHANNELS, out_dev);
}
// ID buffers (ids.hip): RMD_ID_WORDS words a pixel, which is a whole number of doubles
static_assert(RMD_ID_WORDS * sizeof(uint32_t) % sizeof(double) == 0, "an ID record is a whole number of doubles: the framebuffer helpers serve ID buffers");
rmd_status rmd_id_buffer_alloc(rmd_context *ctx, uint32_t width, uint32_t height, uint32_t **out_dev) {
	return alloc_zeroed(ctx, "rmd_id_buffer_alloc: bad argument", width, height, RMD_ID_WORDS * sizeof(uint32_t) / sizeof(double), reinterpret_cast<double **>(out_dev));
}
// AO buffers (ao.hip): RMD_AO_WORDS words a pixel, two doubles
static_assert(RMD_AO_WORDS * sizeof(uint32_t) % sizeof(double) == 0, "an AO record is a whole number of doubles: the framebuffer helpers serve AO buffers");
rmd_status rmd_ao_buffer_alloc(rmd_context *ctx, uint32_t width, uint32_t height, uint32_t **out_dev) {
	return alloc_zeroed(ctx, "rmd_ao_buffer_alloc: bad argument", width, height, RMD_AO_WORDS * sizeof(uint32_t) / sizeof(double), reinterpret_cast<double **>(out_dev));
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

// ---------------------------------------------------------------- tile rectangles <-> packed host buffers
rmd_status rmd_framebuffer_download_tiles_async(rmd_context *ctx, const double *dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects,
                                                uint32_t n_rects, double *host_packed) {
	return rmd::guarded(ctx, "rmd_framebuffer_download_tiles", [&]() -> rmd_status {
		Transfer t;
		if (rmd_status s = begin_transfer(ctx, "rmd_framebuffer_download_tiles", dev, host_packed, width, height, rects, n_rects, t)) return s;
		if (!t.slot) return RMD_OK;
		rmd_context::TransferSlot &sl = *t.slot;
		// main stream: table, pack (behind the renders enqueued before); copy stream: the download (renders enqueued after this overlap it)
		RMD_HIP(ctx, rmd::launch_tile_copy(ctx->stream, true, const_cast<double *>(dev), sl.packed.as<double>(), t.d_rects, t.d_first, n_rects, width));
		RMD_HIP(ctx, hipEventRecord(sl.packed_ready, ctx->stream));
		RMD_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, sl.packed_ready, 0));
		RMD_HIP(ctx, hipMemcpyAsync(host_packed, sl.packed.as<double>(), (size_t)t.n_pixels * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->copy_stream));
		RMD_HIP(ctx, hipEventRecord(sl.copied, ctx->copy_stream));
		sl.in_flight = true;
		return RMD_OK;
	});
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

rmd_status rmd_framebuffer_upload_tiles(rmd_context *ctx, const double *host_packed, double *dev, uint32_t width, uint32_t height,
                                        const rmd_tile_rect *rects, uint32_t n_rects) {
	return rmd::guarded(ctx, "rmd_framebuffer_upload_tiles", [&]() -> rmd_status {
		Transfer t;
		if (rmd_status s = begin_transfer(ctx, "rmd_framebuffer_upload_tiles", dev, host_packed, width, height, rects, n_rects, t)) return s;
		if (!t.slot) return RMD_OK;
		RMD_HIP(ctx, hipMemcpyAsync(t.slot->packed.as<double>(), host_packed, (size_t)t.n_pixels * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
		RMD_HIP(ctx, rmd::launch_tile_copy(ctx->stream, false, dev, t.slot->packed.as<double>(), t.d_rects, t.d_first, n_rects, width));
		RMD_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the caller's buffer and the table are free again
		return rmd::check_fault(ctx); // (this wait has also waited for every render enqueued before it)
	});
}

// ---------------------------------------------------------------- the resolve/tone-map epilogue (kernels.hip: tonemap_kernel; resolve_tiles.hip)
rmd_status rmd_resolve_tonemap(rmd_context *ctx, const double *accum_dev, uint32_t width, uint32_t height, uint32_t sample_count,
                               double exposure, double gamma, uint8_t *out_rgb8_host) {
	return rmd::guarded(ctx, "rmd_resolve_tonemap", [&]() -> rmd_status {
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
		RMD_HIP(ctx, hipMemsetAsync(d_count, 0, 4, ctx->stream));
		RMD_HIP(ctx, rmd::launch_tonemap(ctx->stream, accum_dev, d, n_pixels, sc, exposure, inv_gamma, d_list, d_count));
		return finish_tonemap(ctx, d, n_pixels * 3, d_count, d_list, accum_dev, nullptr, n_pixels * 3, exposure, inv_gamma, out_rgb8_host,
		                      [&](uint32_t i) { return FlaggedPixel{(size_t)i * 3, (size_t)i * 3, sc}; });
	});
}

// The same stage over tile rectangles, each at its own sample count, into rmd_framebuffer_download_tiles's layout (resolve_tiles.hip; the table and
// the way back from a flagged packed pixel: resolve_tiles_host.hpp).  The block's head: [rgb8: 3 P bytes, padded to 16][flag count: 16 bytes]
// [flagged packed pixels: P words, padded to 16].
rmd_status rmd_resolve_tonemap_tiles(rmd_context *ctx, const double *accum_dev, const double *accum2_dev, uint32_t width, uint32_t height,
                                     const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects, double exposure, double gamma,
                                     uint8_t *out_rgb8_host_packed) {
	return rmd::guarded(ctx, "rmd_resolve_tonemap_tiles", [&]() -> rmd_status {
		const std::string name = "rmd_resolve_tonemap_tiles: ";
		if (rmd_status s = bind(ctx)) return s;
		std::vector<uint64_t> first;
		if (rmd_status s = check_run_args(ctx, name, accum_dev, accum2_dev, width, height, rects, rect_sample_counts, n_rects, first)) return s;
		const uint64_t n_pixels = first[n_rects];
		if (n_pixels == 0) return RMD_OK;
		if (!out_rgb8_host_packed) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + "null output for rects that hold pixels");
		const size_t rgb_bytes = ((size_t)n_pixels * 3 + 15) & ~(size_t)15, list_bytes = ((size_t)n_pixels * 4 + 15) & ~(size_t)15;
		rmd::ResolveRun *d_runs = nullptr;
		uint32_t n_runs = 0;
		if (rmd_status s = upload_run_table(ctx, name, rects, rect_sample_counts, n_rects, first, ctx->resolve_tiles, rgb_bytes + 16 + list_bytes, &d_runs, &n_runs)) return s;
		uint8_t *d = ctx->resolve_tiles.block.as<uint8_t>();
		uint32_t *d_count = reinterpret_cast<uint32_t *>(d + rgb_bytes), *d_list = reinterpret_cast<uint32_t *>(d + rgb_bytes + 16);
		const double inv_gamma = 1.0 / gamma;
		RMD_HIP(ctx, hipMemsetAsync(d_count, 0, 4, ctx->stream));
		RMD_HIP(ctx, rmd::launch_resolve_tiles(ctx->stream, accum_dev, accum2_dev, width, d_runs, n_runs, exposure, inv_gamma, d, d_list, d_count));
		return finish_tonemap(ctx, d, (size_t)n_pixels * 3, d_count, d_list, accum_dev, accum2_dev, (size_t)width * height * 3, exposure, inv_gamma, out_rgb8_host_packed,
		                      [&](uint32_t q) {
			                      const rmd::ResolvePixel at = rmd::resolve_locate(rects, n_rects, first, q);
			                      return FlaggedPixel{((size_t)at.x + (size_t)at.y * width) * 3, (size_t)q * 3, (double)rect_sample_counts[at.rect]};
		                      });
	});
}

// The luminance histogram of the same rects (luma_histogram.hip; luma_bins.hpp: the luminance and the counter of a pixel).  The argument rules are
// rmd_resolve_tonemap_tiles's, in its order, and all of them come before the context is looked at.  The block's head: the 261 counters, padded to
// 16 bytes.
static_assert(sizeof(rmd_luma_histogram) == (rmd::kLumaCounters + 1) * sizeof(uint64_t) && RMD_LUMA_BINS == rmd::kLumaBins, "luma_bins.hpp mirrors include/raymond_hip.h");
static_assert(offsetof(rmd_luma_histogram, below) == rmd::kLumaBelow * 8 && offsetof(rmd_luma_histogram, above) == rmd::kLumaAbove * 8 &&
              offsetof(rmd_luma_histogram, zero) == rmd::kLumaZero * 8 && offsetof(rmd_luma_histogram, negative) == rmd::kLumaNegative * 8 &&
              offsetof(rmd_luma_histogram, not_finite) == rmd::kLumaNotFinite * 8 && offsetof(rmd_luma_histogram, pixels) == rmd::kLumaCounters * 8,
              "the device's counters are the struct's fields in order");
rmd_status rmd_luminance_histogram_tiles(rmd_context *ctx, const double *accum_dev, const double *accum2_dev, uint32_t width, uint32_t height,
                                         const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects, rmd_luma_histogram *out_host) {
	return rmd::guarded(ctx, "rmd_luminance_histogram_tiles", [&]() -> rmd_status {
		const std::string name = "rmd_luminance_histogram_tiles: ";
		std::vector<uint64_t> first;
		if (rmd_status s = check_run_args(ctx, name, accum_dev, accum2_dev, width, height, rects, rect_sample_counts, n_rects, first)) return s;
		if (!out_host) return rmd::fail(ctx, RMD_ERR_INVALID_ARGUMENT, name + "null out_host");
		if (rmd_status s = bind(ctx)) return s;
		std::memset(out_host, 0, sizeof(*out_host));
		if (first[n_rects] == 0) return RMD_OK;
		const size_t counter_bytes = ((size_t)rmd::kLumaCounters * sizeof(uint64_t) + 15) & ~(size_t)15;
		rmd::ResolveRun *d_runs = nullptr;
		uint32_t n_runs = 0;
		if (rmd_status s = upload_run_table(ctx, name, rects, rect_sample_counts, n_rects, first, ctx->luma, counter_bytes, &d_runs, &n_runs)) return s;
		uint64_t *d_counters = ctx->luma.block.as<uint64_t>();
		uint64_t counters[rmd::kLumaCounters];
		RMD_HIP(ctx, hipMemsetAsync(d_counters, 0, counter_bytes, ctx->stream));
		RMD_HIP(ctx, rmd::launch_luma_histogram(ctx->stream, accum_dev, accum2_dev, width, d_runs, n_runs, d_counters));
		RMD_HIP(ctx, hipMemcpyAsync(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost, ctx->stream));
		RMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
		std::memcpy(out_host, counters, sizeof(counters)); // (the fields in order: the static_asserts above)
		for (uint32_t i = 0; i < rmd::kLumaCounters; i++) out_host->pixels += counters[i];
		return rmd::check_fault(ctx);
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
