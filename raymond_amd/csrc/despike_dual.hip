// Firefly rejection for the two halves of a dual-buffer frame (rmd_despike_dual; include/raymond_hip.h states the definition, DESIGN.md section 33 the
// structure).  A translation unit of its own: no other unit's code objects change.  The decision is rmd_despike's on the MERGED pixel — despike_rule.hpp's
// functions, unchanged —; the merge, the dual validity and what a half takes from its donor are despike_dual_rule.hpp's, which the C++ mirror and
// tests/despike_dual_rule_main.cpp read as well.
//
// despike_dual_kernel — despike_kernel's shape (despike.hip), its body restated here so that despike.hip's code object stays what it was: one 32 x 16
// output tile per workgroup of 512 threads, one output pixel per thread:
//   1. the apron (tile +- radius, NOT clamped) is staged into LDS as Y and V of the merged pixel, 16 B a pixel — twelve values and two counts are read for
//      each —; a NaN Y marks a position that is no other: outside the frame, or a pixel that is not valid;
//   2. the settle shortcut and 3. the selection behind one branch, exactly despike_kernel's;
//   4. every pixel writes its twelve values: its own bits, or per half the donor's half bits or the donor's per-sample half moments at its own half count;
//   5. the spikes' rect indices meet in LDS; per workgroup and rect touched one lane adds the rect's spikes to the call's counters with one atomic.
// Every decision reads the input alone.  f64 throughout, built with -ffp-contract=off like the rest of the library.
#include <hip/hip_runtime.h>

#include "despike_dual_rule.hpp"
#include "launch.hpp"

namespace rmd {

constexpr int kDespikeDualTileW = 32, kDespikeDualTileH = 16, kDespikeDualThreads = kDespikeDualTileW * kDespikeDualTileH;
constexpr int kDespikeDualApron = (kDespikeDualTileW + 2 * (int)kDespikeMaxRadius) * (kDespikeDualTileH + 2 * (int)kDespikeMaxRadius); // 836 pixels, 13,376 B
constexpr uint32_t kDespikeDualNoRect = 0xFFFFFFFFu;

__global__ __launch_bounds__(kDespikeDualThreads) void despike_dual_kernel(const double *__restrict__ SA, const double *__restrict__ QA, const double *__restrict__ SB,
                                                                            const double *__restrict__ QB, const uint32_t *__restrict__ n_img_a,
                                                                            const uint32_t *__restrict__ n_img_b, const uint32_t *__restrict__ rect_img, uint32_t W,
                                                                            uint32_t H, uint32_t radius, uint32_t rank, double k, double ratio, double floor,
                                                                            double *__restrict__ out_SA, double *__restrict__ out_QA, double *__restrict__ out_SB,
                                                                            double *__restrict__ out_QB, uint32_t *__restrict__ replaced) {
	__shared__ double Ys[kDespikeDualApron], Vs[kDespikeDualApron];
	__shared__ uint32_t spike_rect[kDespikeDualThreads];
	const int r = (int)radius, AW = kDespikeDualTileW + 2 * r, AA = AW * (kDespikeDualTileH + 2 * r);
	const int64_t x0 = (int64_t)blockIdx.x * kDespikeDualTileW, y0 = (int64_t)blockIdx.y * kDespikeDualTileH;
	const int tid = (int)threadIdx.x;

	for (int i = tid; i < AA; i += kDespikeDualThreads) {
		const int ly = i / AW, lx = i - ly * AW;
		const int64_t gx = x0 - r + lx, gy = y0 - r + ly;
		double Y = __builtin_nan(""), V = 0.0;
		if (gx >= 0 && gx < (int64_t)W && gy >= 0 && gy < (int64_t)H) {
			const size_t pix = (size_t)gx + (size_t)gy * W;
			const uint32_t n_a = n_img_a[pix], n_b = n_img_b[pix];
			double sa[3], qa[3], sb[3], qb[3], y, v;
#pragma unroll
			for (int c = 0; c < 3; c++) sa[c] = SA[pix * 3 + c], qa[c] = QA[pix * 3 + c], sb[c] = SB[pix * 3 + c], qb[c] = QB[pix * 3 + c];
			if (despike_dual_pixel(sa, qa, n_a, sb, qb, n_b, y, v)) Y = y, V = v;
		}
		Ys[i] = Y, Vs[i] = V;
	}
	__syncthreads();

	const int tx = tid % kDespikeDualTileW, ty = tid / kDespikeDualTileW;
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

	uint32_t my_rect = kDespikeDualNoRect;
	if (inside) {
		const size_t pix = (size_t)gx + (size_t)gy * W;
		double sa[3], qa[3], sb[3], qb[3];
		if (spike) {
			const size_t dpix = (size_t)(gx + ddx) + (size_t)(gy + ddy) * W; // an other: inside the frame, valid, so both its half counts are >= 1
			const uint32_t n_pa = n_img_a[pix], n_qa = n_img_a[dpix], n_pb = n_img_b[pix], n_qb = n_img_b[dpix];
#pragma unroll
			for (int c = 0; c < 3; c++) {
				sa[c] = despike_dual_take(SA[dpix * 3 + c], n_qa, n_pa), qa[c] = despike_dual_take(QA[dpix * 3 + c], n_qa, n_pa);
				sb[c] = despike_dual_take(SB[dpix * 3 + c], n_qb, n_pb), qb[c] = despike_dual_take(QB[dpix * 3 + c], n_qb, n_pb);
			}
			if (replaced != nullptr) my_rect = rect_img[pix];
		} else {
#pragma unroll
			for (int c = 0; c < 3; c++) sa[c] = SA[pix * 3 + c], qa[c] = QA[pix * 3 + c], sb[c] = SB[pix * 3 + c], qb[c] = QB[pix * 3 + c];
		}
#pragma unroll
		for (int c = 0; c < 3; c++) out_SA[pix * 3 + c] = sa[c], out_QA[pix * 3 + c] = qa[c], out_SB[pix * 3 + c] = sb[c], out_QB[pix * 3 + c] = qb[c];
	}

	if (replaced == nullptr) return; // (the same for every thread)
	spike_rect[tid] = my_rect;
	if (__syncthreads_or(my_rect != kDespikeDualNoRect) == 0) return;
	if (my_rect != kDespikeDualNoRect) {
		// the first of the workgroup's lanes that hold this rect adds for all of them (same-address LDS reads are one broadcast)
		uint32_t n = 0;
		bool first = true;
		for (int j = 0; j < kDespikeDualThreads; j++)
			if (spike_rect[j] == my_rect) {
				if (j < tid) first = false;
				n++;
			}
		if (first) atomicAdd(&replaced[my_rect], n);
	}
}

hipError_t launch_despike_dual(hipStream_t stream, const DenoiseInput &in, uint32_t radius, uint32_t rank, double k, double ratio, double floor, uint32_t *n_img,
                               uint32_t *rect_img, double *out_accum_a, double *out_accum_sq_a, double *out_accum_b, double *out_accum_sq_b, uint32_t *replaced) {
	if (radius < 1u || radius > kDespikeMaxRadius || n_img == nullptr || (replaced != nullptr && rect_img == nullptr)) return hipErrorInvalidValue;
	const size_t N = (size_t)in.W * in.H;
	DenoiseInput half_b = in; // the count image's launcher paints counts_a
	half_b.counts_a = in.counts_b;
	hipError_t e = launch_denoise_planes(stream, in, n_img, nullptr); // half A's count image: zeroed, then painted rect by rect
	if (e != hipSuccess) return e;
	if ((e = launch_denoise_planes(stream, half_b, n_img + N, nullptr)) != hipSuccess) return e; // half B's
	if (replaced != nullptr && in.n_rects != 0u)
		if ((e = launch_rect_index_image(stream, in, rect_img, replaced)) != hipSuccess) return e;
	const dim3 grid((in.W + kDespikeDualTileW - 1u) / kDespikeDualTileW, (in.H + kDespikeDualTileH - 1u) / kDespikeDualTileH);
	hipLaunchKernelGGL(despike_dual_kernel, grid, dim3(kDespikeDualThreads), 0, stream, in.accum_a, in.accum_sq_a, in.accum_b, in.accum_sq_b, n_img, n_img + N, rect_img,
	                   in.W, in.H, radius, rank, k, ratio, floor, out_accum_a, out_accum_sq_a, out_accum_b, out_accum_sq_b, in.n_rects != 0u ? replaced : nullptr);
	return hipGetLastError();
}

} // namespace rmd
