// Firefly rejection from the moments (rmd_despike; include/raymond_hip.h states the definition, DESIGN.md section 24 the structure).  A translation unit
// of its own: no other unit's code objects change.  The rule — Y, V, the order of the others, the spike test, the scaled copy — is despike_rule.hpp's,
// which the C++ mirror and tests/despike_rule_main.cpp read as well.
//
// rect_index_image_kernel — count_image_kernel's (denoise.hip) twin for the rect's INDEX: which rect a spike is counted in.  Pixels no rect covers are not
//                           painted and never read: a spike is valid, so a rect covers it.
// despike_kernel          — one 32 x 16 output tile per workgroup of 512 threads, one output pixel per thread:
//   1. the apron (tile +- radius, NOT clamped) is staged into LDS as Y and V, 16 B a pixel; a NaN Y marks a position that is no other — outside the frame,
//      or a pixel that is not valid (Y of a valid pixel is never NaN: its means are finite);
//   2. every valid pixel counts the others at or above its own Y: more than `rank` of them with Y_p >= 0 settle it (despike_settled) — every pixel of
//      non-negative luminance but its window's top rank + 1 —, and a wave whose lanes are all settled skips the selection as one branch;
//   3. the rest — the local top rank + 1, and every pixel of negative luminance — select their donor in rank + 1 passes over the window and take the test;
//   4. every pixel writes its six values: its own bits, the donor's bits, or the donor's per-sample moments at its own count;
//   5. the spikes' rect indices meet in LDS; per workgroup and rect touched one lane adds the rect's spikes to the call's counters with one atomic.
// Every decision reads the input alone.  f64 throughout, built with -ffp-contract=off like the rest of the library.
#include <hip/hip_runtime.h>

#include "despike_rule.hpp"
#include "launch.hpp"

namespace rmd {

constexpr int kDespikeTileW = 32, kDespikeTileH = 16, kDespikeThreads = kDespikeTileW * kDespikeTileH;
constexpr int kDespikeApron = (kDespikeTileW + 2 * (int)kDespikeMaxRadius) * (kDespikeTileH + 2 * (int)kDespikeMaxRadius); // 836 pixels, 13,376 B
constexpr uint32_t kDespikeNoRect = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void rect_index_image_kernel(const rmd_tile_rect *__restrict__ rects, uint32_t W, uint32_t *__restrict__ rect_img) {
	const rmd_tile_rect r = rects[blockIdx.x];
	const uint64_t n_px = (uint64_t)r.width * r.height;
	for (uint64_t i = (uint64_t)blockIdx.y * 256u + threadIdx.x; i < n_px; i += (uint64_t)gridDim.y * 256u) {
		const uint32_t x = (uint32_t)(i % r.width), y = (uint32_t)(i / r.width);
		rect_img[(size_t)(r.left + x) + (size_t)(r.top + y) * W] = blockIdx.x;
	}
}

__global__ __launch_bounds__(kDespikeThreads) void despike_kernel(const double *__restrict__ S, const double *__restrict__ Q, const uint32_t *__restrict__ n_img,
                                                                   const uint32_t *__restrict__ rect_img, uint32_t W, uint32_t H, uint32_t radius, uint32_t rank,
                                                                   double k, double ratio, double floor, double *__restrict__ out_S, double *__restrict__ out_Q,
                                                                   uint32_t *__restrict__ replaced) {
	__shared__ double Ys[kDespikeApron], Vs[kDespikeApron];
	__shared__ uint32_t spike_rect[kDespikeThreads];
	const int r = (int)radius, AW = kDespikeTileW + 2 * r, AA = AW * (kDespikeTileH + 2 * r);
	const int64_t x0 = (int64_t)blockIdx.x * kDespikeTileW, y0 = (int64_t)blockIdx.y * kDespikeTileH;
	const int tid = (int)threadIdx.x;

	for (int i = tid; i < AA; i += kDespikeThreads) {
		const int ly = i / AW, lx = i - ly * AW;
		const int64_t gx = x0 - r + lx, gy = y0 - r + ly;
		double Y = __builtin_nan(""), V = 0.0;
		if (gx >= 0 && gx < (int64_t)W && gy >= 0 && gy < (int64_t)H) {
			const size_t pix = (size_t)gx + (size_t)gy * W;
			const uint32_t n = n_img[pix];
			double s[3], q[3], y, v;
#pragma unroll
			for (int c = 0; c < 3; c++) s[c] = S[pix * 3 + c], q[c] = Q[pix * 3 + c];
			if (despike_pixel(s, q, n, y, v)) Y = y, V = v;
		}
		Ys[i] = Y, Vs[i] = V;
	}
	__syncthreads();

	const int tx = tid % kDespikeTileW, ty = tid / kDespikeTileW;
	const int64_t gx = x0 + tx, gy = y0 + ty;
	const bool inside = gx < (int64_t)W && gy < (int64_t)H;
	const int centre = (ty + r) * AW + (tx + r);
	const double *win = Ys + (centre - r * AW - r); // the window's first row and column: inside the apron for every thread of the tile
	const double yp = Ys[centre];
	bool spike = false;
	int ddx = 0, ddy = 0;
	if (inside && yp == yp && !despike_settled(despike_at_or_above(win, (uint32_t)AW, radius, yp), rank, yp)) {
		const int donor = despike_donor(win, (uint32_t)AW, radius, rank);
		if (donor >= 0) {
			const int side = 2 * r + 1;
			ddy = donor / side - r, ddx = donor % side - r;
			const int at = centre + ddy * AW + ddx;
			spike = despike_is_spike(yp, Ys[at], Vs[at], k, ratio, floor);
		}
	}

	uint32_t my_rect = kDespikeNoRect;
	if (inside) {
		const size_t pix = (size_t)gx + (size_t)gy * W;
		double s[3], q[3];
		if (spike) {
			const size_t dpix = (size_t)(gx + ddx) + (size_t)(gy + ddy) * W; // an other: inside the frame
			const uint32_t n_p = n_img[pix], n_q = n_img[dpix];
#pragma unroll
			for (int c = 0; c < 3; c++) {
				s[c] = S[dpix * 3 + c], q[c] = Q[dpix * 3 + c];
				if (n_p != n_q) s[c] = despike_scaled(s[c], n_q, n_p), q[c] = despike_scaled(q[c], n_q, n_p);
			}
			if (replaced != nullptr) my_rect = rect_img[pix];
		} else {
#pragma unroll
			for (int c = 0; c < 3; c++) s[c] = S[pix * 3 + c], q[c] = Q[pix * 3 + c];
		}
#pragma unroll
		for (int c = 0; c < 3; c++) out_S[pix * 3 + c] = s[c], out_Q[pix * 3 + c] = q[c];
	}

	if (replaced == nullptr) return; // (the same for every thread)
	spike_rect[tid] = my_rect;
	if (__syncthreads_or(my_rect != kDespikeNoRect) == 0) return;
	if (my_rect != kDespikeNoRect) {
		// the first of the workgroup's lanes that hold this rect adds for all of them (same-address LDS reads are one broadcast)
		uint32_t n = 0;
		bool first = true;
		for (int j = 0; j < kDespikeThreads; j++)
			if (spike_rect[j] == my_rect) {
				if (j < tid) first = false;
				n++;
			}
		if (first) atomicAdd(&replaced[my_rect], n);
	}
}

hipError_t launch_rect_index_image(hipStream_t stream, const DenoiseInput &in, uint32_t *rect_img, uint32_t *replaced) {
	hipError_t e = hipMemsetAsync(replaced, 0, (size_t)in.n_rects * sizeof(uint32_t), stream);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(rect_index_image_kernel, dim3(in.n_rects, in.count_image_columns), dim3(256), 0, stream, in.rects, in.W, rect_img);
	return hipGetLastError();
}

hipError_t launch_despike(hipStream_t stream, const DenoiseInput &in, uint32_t radius, uint32_t rank, double k, double ratio, double floor, uint32_t *n_img,
                          uint32_t *rect_img, double *out_accum, double *out_accum_sq, uint32_t *replaced) {
	if (radius < 1u || radius > kDespikeMaxRadius || n_img == nullptr || (replaced != nullptr && rect_img == nullptr)) return hipErrorInvalidValue;
	hipError_t e = launch_denoise_planes(stream, in, n_img, nullptr); // the count image: zeroed, then painted rect by rect
	if (e != hipSuccess) return e;
	if (replaced != nullptr && in.n_rects != 0u)
		if ((e = launch_rect_index_image(stream, in, rect_img, replaced)) != hipSuccess) return e;
	const dim3 grid((in.W + kDespikeTileW - 1u) / kDespikeTileW, (in.H + kDespikeTileH - 1u) / kDespikeTileH);
	hipLaunchKernelGGL(despike_kernel, grid, dim3(kDespikeThreads), 0, stream, in.accum_a, in.accum_sq_a, n_img, rect_img, in.W, in.H, radius, rank, k, ratio, floor,
	                   out_accum, out_accum_sq, in.n_rects != 0u ? replaced : nullptr);
	return hipGetLastError();
}

} // namespace rmd
