// HIP kernels of the radiance integrator for gfx950 (CDNA4).
//
// render_kernel<MODE=tiles|tiles-buffered, GRID, PERSIST> — the hot path (render_kernel.hpp).  Persistent 16-wave workgroups, one per CU, whose
//   waves draw (8x8 wave tile, sample range) work items from a counter.  trace()'s recursion (src/trace.rs:232-320) becomes a running
//   throughput: each bounce's weight is multiplied in when it is produced and the terminal radiance is scaled by the product (DESIGN.md
//   section 3).  The object table is staged into LDS once per workgroup; the uniform closest-hit loop reads it through scalar loads, the
//   divergent post-hit lookup reads the LDS copy.  Two wave bodies:
//     render_wave_sorted (split launches of scenes without grids — the spheres kernel): the wave's paths live in a pool of slots in LDS and a trip is
//       64 new samples (primary ray, intersection, classification) or 64 parked hits (shading, intersection, classification): every lane
//       of a trip needs the same thing;
//     render_wave (everything else): a lane keeps its path and regenerates the next sample's primary ray in place; GRID = true adds the
//       wave-cooperative grid walk (grid_walk.hpp) and shares the grids' occupancy masks through LDS.
//   MFMA is not used: there is no dense contraction anywhere on this path.
// (The kernel template itself is in render_kernel.hpp; its list instantiation — an explicit (x, y, sample) per lane, for the
// parity probes — and the probe kernels are compiled into libraymond_hip_probe.so from probe_kernels.hip, not into this library.)
// sum_kernel, tonemap_kernel — the ordered per-sample sum of split launches of mesh scenes (the spheres kernel does it itself) and
// the output stage.
#include <hip/hip_runtime.h>

#include "render_kernel.hpp"

namespace rmd {

// Second half of a split launch: pixel += sample(s) for s = sample_begin .. +sample_count-1, strictly in that order
// (src/trace.rs:203), reading the per-sample radiance the render kernel stored.  One wavefront per wave tile, lane = pixel;
// every load is 24 contiguous bytes per lane, 1.5 KiB contiguous per wave.
__global__ __launch_bounds__(64) void sum_kernel(RenderParams P, const WaveTile *__restrict__ tiles, const double *__restrict__ buf,
                                                 double *__restrict__ out) {
	const uint32_t wt = blockIdx.x, lane = threadIdx.x;
	const WaveTile t = tiles[wt];
	const uint32_t lx = lane & 7u, ly = lane >> 3;
	if (lx >= t.w || ly >= t.h) return;
	const size_t pix = ((size_t)(t.x0 + lx) + (size_t)(t.y0 + ly) * P.W) * 3;
	V3 acc = ld3(out + pix);
	const double *src = buf + ((size_t)wt * P.sample_count * 64u + lane) * kSampleStride;
	for (uint32_t s = 0; s < P.sample_count; s++) {
		acc = acc + ld3(src);
		src += 64u * kSampleStride;
	}
	out[pix + 0] = acc.x, out[pix + 1] = acc.y, out[pix + 2] = acc.z;
}

// The same sum for rmd_render_tiles_moments: out_sq += sample(s)^2 per channel beside it, same samples, same order — the square rounded, then
// added.  (A kernel of its own: sum_kernel stays exactly what a render without moments runs.)
__global__ __launch_bounds__(64) void sum_moments_kernel(RenderParams P, const WaveTile *__restrict__ tiles, const double *__restrict__ buf,
                                                         double *__restrict__ out, double *__restrict__ out_sq) {
	const uint32_t wt = blockIdx.x, lane = threadIdx.x;
	const WaveTile t = tiles[wt];
	const uint32_t lx = lane & 7u, ly = lane >> 3;
	if (lx >= t.w || ly >= t.h) return;
	const size_t pix = ((size_t)(t.x0 + lx) + (size_t)(t.y0 + ly) * P.W) * 3;
	V3 acc = ld3(out + pix), sq = ld3(out_sq + pix);
	const double *src = buf + ((size_t)wt * P.sample_count * 64u + lane) * kSampleStride;
	for (uint32_t s = 0; s < P.sample_count; s++) {
		const V3 v = ld3(src);
		acc = acc + v;
		sq = sq + hadamard(v, v);
		src += 64u * kSampleStride;
	}
	out[pix + 0] = acc.x, out[pix + 1] = acc.y, out[pix + 2] = acc.z;
	out_sq[pix + 0] = sq.x, out_sq[pix + 1] = sq.y, out_sq[pix + 2] = sq.z;
}

// ---------------------------------------------------------------- per-tile error (rmd_tile_error)
// One workgroup per rect, striding over its pixels.  For n samples, S = accum, Q = accum_sq, per channel:
//     m = S / n;  v = (Q - S*m) / (n - 1), 0 if negative;  e_c = sqrt(v / n) / max(|m|, floor)
// a pixel's error is its largest e_c (+inf when one of its S or Q is not finite, or n < 2), the rect's the largest of its pixels'.  A maximum
// is the same whatever order it is taken in: the result does not depend on how the pixels are dealt to lanes.  (With finite inputs and a
// floor > 0 no e_c is NaN: S*m >= 0, so Q - S*m cannot overflow upwards, and an overflow of S*m makes v -inf, which is clamped.)
__global__ __launch_bounds__(256) void tile_error_kernel(const double *__restrict__ S, const double *__restrict__ Q, const rmd_tile_rect *__restrict__ rects,
                                                          uint32_t W, uint32_t n, double floor, double *__restrict__ out) {
	const rmd_tile_rect r = rects[blockIdx.x];
	const uint64_t n_px = (uint64_t)r.width * r.height;
	const double nd = (double)n;
	double e = 0.0;
	for (uint64_t i = threadIdx.x; i < n_px; i += 256u) {
		const uint32_t x = (uint32_t)(i % r.width), y = (uint32_t)(i / r.width);
		const size_t p = ((size_t)(r.left + x) + (size_t)(r.top + y) * W) * 3;
		bool bad = n < 2u;
		double ep = 0.0;
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const double s = S[p + c], q = Q[p + c];
			bad = bad || !(__builtin_fabs(s) < __builtin_inf()) || !(__builtin_fabs(q) < __builtin_inf());
			const double m = s / nd;
			double v = (q - s * m) / (nd - 1.0);
			if (v < 0.0) v = 0.0;
			const double ec = __builtin_sqrt(v / nd) / __builtin_fmax(__builtin_fabs(m), floor);
			ep = __builtin_fmax(ep, ec);
		}
		e = __builtin_fmax(e, bad ? __builtin_inf() : ep);
	}
	for (int off = 32; off > 0; off >>= 1) e = __builtin_fmax(e, __shfl_xor(e, off, 64));
	__shared__ double wave_max[4];
	if ((threadIdx.x & 63u) == 0u) wave_max[threadIdx.x >> 6] = e;
	__syncthreads();
	if (threadIdx.x == 0u) out[blockIdx.x] = __builtin_fmax(__builtin_fmax(wave_max[0], wave_max[1]), __builtin_fmax(wave_max[2], wave_max[3]));
}
hipError_t launch_tile_error(hipStream_t stream, const double *accum, const double *accum_sq, const rmd_tile_rect *rects, uint32_t n_rects, uint32_t W,
                             uint32_t sample_count, double floor, double *out) {
	if (n_rects == 0) return hipSuccess;
	hipLaunchKernelGGL(tile_error_kernel, dim3(n_rects), dim3(256), 0, stream, accum, accum_sq, rects, W, sample_count, floor, out);
	return hipGetLastError();
}

// ---------------------------------------------------------------- resolve + tone-map (cli_old/src/main.rs:161-181, src/trace.rs:95)
// The reference's 8-bit value is trunc(255 * (1 - exp(-p * exposure))^(1/gamma)) with the HOST libm's exp and powf.  The device's exp / pow
// differ from a host libm by an ulp or two, which can only change the byte when 255 * tm lies within a few 1e-13 of an integer.  So the
// kernel computes every pixel and FLAGS the few whose value is within kTonemapGuard of a truncation boundary (1 .. 255); the host
// recomputes exactly those with its libm (api_frame.cpp: rmd_resolve_tonemap) — byte-exact output, and a pixel in ~10^6 takes the slow road.
// Two exact cases need no flag: an argument <= -40 gives exp < 2^-57, 1 - exp = 1, pow(1, y) = 1 and 255 exactly with ANY libm
// (saturated pixels); and values that truncate to 0 either way (|255 tm| < 1 - guard: black pixels).
__global__ __launch_bounds__(256) void tonemap_kernel(const double *__restrict__ accum, uint8_t *__restrict__ rgb8, size_t n_pixels,
                                                       double sample_count, double exposure, double inv_gamma, uint32_t *__restrict__ flagged,
                                                       uint32_t *__restrict__ n_flagged) {
	size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_pixels) return;
	double v[3];
	bool ok = true, flag = false;
#pragma unroll
	for (int c = 0; c < 3; c++) {
		double p = accum[i * 3 + c] / sample_count; // TaskHandle::await, src/trace.rs:95
		const double arg = p * -1.0 * exposure;
		double tm = 1.0 - exp(arg);
		tm = pow(tm, inv_gamma);
		v[c] = tm * 255.0;
		ok = ok && (v[c] > -1.0 && v[c] < 256.0);
		const double r = __builtin_rint(v[c]);
		flag = flag || (r >= 1.0 && __builtin_fabs(v[c] - r) < kTonemapGuard && !(arg <= -40.0));
	}
	// Vector3<f64>.cast::<u8>() is None if any channel is NaN / out of range: the pixel then stays (0,0,0)
#pragma unroll
	for (int c = 0; c < 3; c++) rgb8[i * 3 + c] = ok ? (uint8_t)v[c] : (uint8_t)0;
	if (flag) flagged[atomicAdd(n_flagged, 1u)] = (uint32_t)i; // the list has room for every pixel
}

// ---------------------------------------------------------------- tile rectangles <-> a packed buffer (rmd_framebuffer_{download,upload}_tiles)
// One workgroup per rectangle; rect i's pixels row-major at packed + first[i] * 3 — the layout of core::tile::Tile.data (core/src/tile.rs:13).
// Every access is 24 contiguous bytes per lane, a row of the rectangle (<= 32 pixels = 768 bytes) contiguous on both sides.
template <bool TO_PACKED>
__global__ __launch_bounds__(256) void tile_copy_kernel(double *__restrict__ frame, double *__restrict__ packed, const rmd_tile_rect *__restrict__ rects,
                                                         const uint64_t *__restrict__ first, uint32_t W) {
	const rmd_tile_rect r = rects[blockIdx.x];
	const uint64_t base = first[blockIdx.x];
	const uint32_t n = r.width * r.height;
	for (uint32_t i = threadIdx.x; i < n; i += 256u) {
		const uint32_t x = i % r.width, y = i / r.width;
		double *f = frame + ((size_t)(r.left + x) + (size_t)(r.top + y) * W) * 3, *p = packed + (base + i) * 3;
		if (TO_PACKED) p[0] = f[0], p[1] = f[1], p[2] = f[2];
		else f[0] = p[0], f[1] = p[1], f[2] = p[2];
	}
}
hipError_t launch_tile_copy(hipStream_t stream, bool to_packed, double *frame, double *packed, const rmd_tile_rect *rects, const uint64_t *first,
                            uint32_t n_rects, uint32_t W) {
	if (n_rects == 0) return hipSuccess;
	if (to_packed) hipLaunchKernelGGL(tile_copy_kernel<true>, dim3(n_rects), dim3(256), 0, stream, frame, packed, rects, first, W);
	else hipLaunchKernelGGL(tile_copy_kernel<false>, dim3(n_rects), dim3(256), 0, stream, frame, packed, rects, first, W);
	return hipGetLastError();
}

// ---------------------------------------------------------------- launchers
size_t render_lds_bytes(uint32_t n_objects, uint32_t mask_words_total, uint32_t waves_per_wg) {
	// a scene has grids exactly when it has mask words reserved (an all-empty grid still reserves some)
	return (size_t)n_objects * sizeof(DevObject) + (size_t)((mask_words_total + 3u) & ~3u) * 4u +
	       (size_t)waves_per_wg * wave_lds_bytes(mask_words_total ? 1u : 0u);
}

LaunchPlan plan_render_launch(int mode, bool grid, uint32_t n_objects, uint32_t mask_words_total, bool queues, bool persist, bool chain_items, bool moments,
                              uint32_t n_waves, uint32_t n_cus) {
	switch (mode * 2 + (grid ? 1 : 0)) {
	case kModeTiles * 2: return plan_launch<kModeTiles, false>(n_objects, mask_words_total, queues, persist, chain_items, moments, n_waves, n_cus);
	case kModeTiles * 2 + 1: return plan_launch<kModeTiles, true>(n_objects, mask_words_total, queues, persist, chain_items, moments, n_waves, n_cus);
	case kModeTilesBuffered * 2: return plan_launch<kModeTilesBuffered, false>(n_objects, mask_words_total, queues, persist, chain_items, moments, n_waves, n_cus);
	case kModeTilesBuffered * 2 + 1: return plan_launch<kModeTilesBuffered, true>(n_objects, mask_words_total, queues, persist, chain_items, moments, n_waves, n_cus);
	case kModeList * 2: return plan_launch<kModeList, false>(n_objects, mask_words_total, queues, persist, chain_items, moments, n_waves, n_cus);
	case kModeList * 2 + 1: return plan_launch<kModeList, true>(n_objects, mask_words_total, queues, persist, chain_items, moments, n_waves, n_cus);
	}
	return LaunchPlan{};
}

template <int MODE, bool GRID>
static void lds_sizes_of(uint64_t out[8]) {
	out[0] = kLdsBudgetBytes, out[1] = sizeof(DevObject), out[2] = wave_lds_of<MODE, GRID>(GRID ? 1u : 0u), out[3] = queued_wave_lds_bytes();
	out[4] = kPersistWaves<MODE, GRID>, out[5] = kGridWavesPerWg, out[6] = kSortPoolBytes, out[7] = kMaskBudgetBytes;
}
void render_lds_sizes(int mode, bool grid, uint64_t out[8]) {
	switch (mode * 2 + (grid ? 1 : 0)) {
	case kModeTiles * 2: return lds_sizes_of<kModeTiles, false>(out);
	case kModeTiles * 2 + 1: return lds_sizes_of<kModeTiles, true>(out);
	case kModeTilesBuffered * 2: return lds_sizes_of<kModeTilesBuffered, false>(out);
	case kModeTilesBuffered * 2 + 1: return lds_sizes_of<kModeTilesBuffered, true>(out);
	case kModeList * 2: return lds_sizes_of<kModeList, false>(out);
	case kModeList * 2 + 1: return lds_sizes_of<kModeList, true>(out);
	}
	for (int i = 0; i < 8; i++) out[i] = 0;
}

hipError_t launch_render_tiles(hipStream_t stream, const RenderParams &P, const DevObject *objs, const DevGrid *grids,
                               const WaveTile *wave_tiles, double *accum, uint32_t n_cus, LaunchShape *shape, double *accum_sq) {
	if (P.n_work == 0) return hipSuccess;
	const bool buffered = P.buffered != 0u;
	const uint32_t n_waves = buffered ? work_list_items(P.n_work, P.n_whole, P.split_k) : P.n_work;
	hipError_t e;
	if (P.n_grids) e = buffered ? launch_render<kModeTilesBuffered, true>(stream, P, objs, grids, wave_tiles, n_waves, accum, nullptr, nullptr, n_cus, shape)
	                            : launch_render<kModeTiles, true>(stream, P, objs, grids, wave_tiles, n_waves, accum, nullptr, nullptr, n_cus, shape, accum_sq);
	else e = buffered ? launch_render<kModeTilesBuffered, false>(stream, P, objs, grids, wave_tiles, n_waves, accum, nullptr, nullptr, n_cus, shape, accum_sq)
	                  : launch_render<kModeTiles, false>(stream, P, objs, grids, wave_tiles, n_waves, accum, nullptr, nullptr, n_cus, shape, accum_sq);
	if (e != hipSuccess || !buffered || P.tile_done != nullptr) return e; // with tile_done the render kernel's waves add the samples themselves
	if (accum_sq) hipLaunchKernelGGL(sum_moments_kernel, dim3(P.n_work), dim3(64), 0, stream, P, wave_tiles, (const double *)P.sample_buf, accum, accum_sq);
	else hipLaunchKernelGGL(sum_kernel, dim3(P.n_work), dim3(64), 0, stream, P, wave_tiles, (const double *)P.sample_buf, accum);
	return hipGetLastError();
}

hipError_t launch_sum(hipStream_t stream, const RenderParams &P, const WaveTile *wave_tiles, double *accum) {
	if (P.n_work == 0) return hipSuccess;
	hipLaunchKernelGGL(sum_kernel, dim3(P.n_work), dim3(64), 0, stream, P, wave_tiles, (const double *)P.sample_buf, accum);
	return hipGetLastError();
}

hipError_t launch_tonemap(hipStream_t stream, const double *accum, uint8_t *rgb8, size_t n, double sample_count, double exposure,
                          double inv_gamma, uint32_t *flagged, uint32_t *n_flagged) {
	// n = number of pixels; flagged: n entries, n_flagged: one zeroed word
	if (n == 0) return hipSuccess;
	hipLaunchKernelGGL(tonemap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, accum, rgb8, n, sample_count, exposure,
	                   inv_gamma, flagged, n_flagged);
	return hipGetLastError();
}

} // namespace rmd
