// The edge-avoiding a-trous filter on two sample halves, each filtered with the weights of the other, and its per-pixel error estimate
// (rmd_denoise_atrous_dual; include/raymond_hip.h states the definition, DESIGN.md section 18 the structure and its cost).  A translation unit of
// its own: no other unit's code objects change.
//
// The state is denoise_dual.hip's twelve planes (launch_dual_planes: half h's c in planes 6h + c, its v in planes 6h + 3 + c, a NaN in plane 0 at a
// pixel that is not dual-valid), twice: the levels alternate between the two sets.  The count images and the fourteen feature planes at the
// features' own count are that unit's too.
// atrous_dual_level_kernel<G, LAST> — one level of BOTH cross passes: one thread per pixel, 64 x 4 pixels per workgroup, the 25 taps at step s read
//                                     straight from the planar images in global memory, no LDS, tap loops rolled (atrous_level_kernel's shape,
//                                     denoise_atrous.hip).  Per taken tap the thread reads q's twelve state values once, makes the feature weight
//                                     once (G: guided) and uses it in both passes, and makes two colour distances and two exp: w_B from
//                                     (c_B, v_B) weighs half A's values, w_A from (c_A, v_A) half B's.  LAST = false writes the other set of
//                                     twelve planes; LAST = true writes out_dev and err_dev (rmd_denoise_dual's combination of f_A and f_B), and
//                                     the merged mean and NaN for a pixel that is not dual-valid.
// atrous_dual_mean_kernel           — levels = 0: the same combination of u_A and u_B.
// REGION (rmd_denoise_atrous_dual_region): atrous_dual_level_kernel<G, LAST, true> takes one more trailing argument, a block
//                                     table (launch.hpp: DualBlock), and workgroup b owns the 64 x 4 pixels at entry b's origin that lie before its far
//                                     corner; nothing else differs, so a pixel's value is the whole-frame call's.  The whole-frame instantiations
//                                     keep their arguments and their instructions.  atrous_dual_mean_region_kernel is the closed form and
//                                     atrous_dual_planes_region_kernel<G> the prologue (the pixel functions of denoise_dual.hip's dual_planes_kernel
//                                     and dual_feature_planes_kernel, in one pass) over a block table's pixels.  The host makes one table per
//                                     kernel from the needed sets (launch_denoise_atrous_dual_region).
// SLOPE (rmd_denoise_atrous_dual_slope[_region] at slope > 0): one more trailing argument, last, the seven planes m of the f planes'
//                                     slope floors; the kernel reads p's seven m once, where the denominators are made, and the same m serves every
//                                     level and both passes.  The whole-frame call makes them with denoise.hip's feature_slope_kernel
//                                     (launch_feature_slope); the region call with atrous_dual_slope_region_kernel, the same pixel function over level
//                                     0's block table — every level's pixels lie in it, and the prologue's table holds their neighbours' f.  The
//                                     instantiations without the argument keep their arguments and their instructions.
// The per-pixel arithmetic and rmd_denoise_dual's combination are denoise_device.hpp's.
// f64 throughout, built with -ffp-contract=off like the rest of the library.
#include <hip/hip_runtime.h>

#include "denoise_device.hpp"

namespace rmd {

constexpr int kAtrousDualBlockW = 64, kAtrousDualBlockH = 4;

// levels = 0 at pixel i: the combination of u_A and u_B, the merged mean at a pixel that is not dual-valid
__device__ inline void atrous_dual_mean_pixel(const double *__restrict__ planes, const double *__restrict__ SA, const double *__restrict__ SB,
                                              const uint32_t *__restrict__ n_a, const uint32_t *__restrict__ n_b, size_t i, size_t N, double *__restrict__ out,
                                              double *__restrict__ err) {
	const double na = (double)n_a[i], nb = (double)n_b[i];
	const double a0 = planes[i];
	if (a0 == a0) {
		const double a[3] = {a0, planes[N + i], planes[2 * N + i]}, b[3] = {planes[6 * N + i], planes[7 * N + i], planes[8 * N + i]};
		dual_combine(a, b, na, nb, i, out, err);
	} else {
		dual_merged(SA, SB, na, nb, i, out, err);
	}
}

__global__ __launch_bounds__(256) void atrous_dual_mean_kernel(const double *__restrict__ planes, const double *__restrict__ SA, const double *__restrict__ SB,
                                                               const uint32_t *__restrict__ n_a, const uint32_t *__restrict__ n_b, size_t N, double *__restrict__ out,
                                                               double *__restrict__ err) {
	const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i < N) atrous_dual_mean_pixel(planes, SA, SB, n_a, n_b, i, N, out, err);
}

// The region call's count images: dual_count_image_kernel and dual_feature_count_image_kernel of denoise_dual.hip in one pass (n_a, n_b and n_f are
// zeroed by the caller; counts_f and n_f are null without the guide)
__global__ __launch_bounds__(256) void atrous_dual_count_image_kernel(const rmd_tile_rect *__restrict__ rects, const uint32_t *__restrict__ counts_a,
                                                                      const uint32_t *__restrict__ counts_b, const uint32_t *__restrict__ counts_f, uint32_t W,
                                                                      uint32_t *__restrict__ n_a, uint32_t *__restrict__ n_b, uint32_t *__restrict__ n_f) {
	const rmd_tile_rect r = rects[blockIdx.x];
	const uint32_t na = counts_a[blockIdx.x], nb = counts_b[blockIdx.x], nf = counts_f ? counts_f[blockIdx.x] : 0u;
	const uint64_t n_px = (uint64_t)r.width * r.height;
	for (uint64_t i = (uint64_t)blockIdx.y * 256u + threadIdx.x; i < n_px; i += (uint64_t)gridDim.y * 256u) {
		const size_t p = rect_pixel(r, i, W);
		n_a[p] = na, n_b[p] = nb;
		if (n_f) n_f[p] = nf;
	}
}

// ... over a block table's pixels: workgroup b owns the 64 x 4 pixels at entry b's origin that lie before its far corner
__global__ __launch_bounds__(256) void atrous_dual_mean_region_kernel(const double *__restrict__ planes, const double *__restrict__ SA, const double *__restrict__ SB,
                                                                      const uint32_t *__restrict__ n_a, const uint32_t *__restrict__ n_b,
                                                                      const DualBlock *__restrict__ table, uint32_t W, size_t N, double *__restrict__ out,
                                                                      double *__restrict__ err) {
	const DualBlock e = table[blockIdx.x];
	const uint32_t x = e.x0 + threadIdx.x % kAtrousDualBlockW, y = e.y0 + threadIdx.x / kAtrousDualBlockW; // (no wrap: the origin lies before the far corner)
	if (x < e.x_end && y < e.y_end) atrous_dual_mean_pixel(planes, SA, SB, n_a, n_b, (size_t)x + (size_t)y * W, N, out, err);
}

// The prologue over a block table's pixels: dual_planes_kernel's twelve planes and, GUIDED, dual_feature_planes_kernel's fourteen (denoise_dual.hip) —
// a pixel's feature validity reads only its own dual validity, so one thread makes both.
template <bool GUIDED>
__global__ __launch_bounds__(256) void atrous_dual_planes_region_kernel(const double *__restrict__ SA, const double *__restrict__ QA, const double *__restrict__ SB,
                                                                        const double *__restrict__ QB, const double *__restrict__ F, const double *__restrict__ G,
                                                                        const uint32_t *__restrict__ n_a, const uint32_t *__restrict__ n_b,
                                                                        const uint32_t *__restrict__ n_f, const DualBlock *__restrict__ table, uint32_t W, size_t N,
                                                                        double *__restrict__ planes, double *__restrict__ fplanes) {
	const DualBlock e = table[blockIdx.x];
	const uint32_t x = e.x0 + threadIdx.x % kAtrousDualBlockW, y = e.y0 + threadIdx.x / kAtrousDualBlockW;
	if (x >= e.x_end || y >= e.y_end) return;
	const size_t i = (size_t)x + (size_t)y * W;
	const bool dual = dual_planes_pixel(SA, QA, SB, QB, n_a[i], n_b[i], i, N, planes);
	if constexpr (GUIDED) feature_planes_pixel(F, G, i, n_f[i], dual, N, fplanes);
}

// The slope floors over a block table's pixels (the region _slope call: level 0's table): feature_slope_pixel with the FRAME's width and height, so a
// neighbour is present exactly when the whole-frame call finds it so — inside the frame and feature-valid, whatever the table holds
__global__ __launch_bounds__(256) void atrous_dual_slope_region_kernel(const double *__restrict__ fplanes, const DualBlock *__restrict__ table, uint32_t W, uint32_t H,
                                                                       size_t N, double s2, double *__restrict__ mplanes) {
	const DualBlock e = table[blockIdx.x];
	const uint32_t x = e.x0 + threadIdx.x % kAtrousDualBlockW, y = e.y0 + threadIdx.x / kAtrousDualBlockW;
	if (x < e.x_end && y < e.y_end) feature_slope_pixel(fplanes, (size_t)x + (size_t)y * W, x, y, W, H, N, s2, mplanes);
}

// the trailing arguments: the block table (REGION), then the slope planes (SLOPE)
__device__ inline const DualBlock *atrous_dual_table(const DualBlock *t) { return t; }
__device__ inline const DualBlock *atrous_dual_table(const DualBlock *t, const double *) { return t; }
__device__ inline const double *atrous_dual_slope(const double *m) { return m; }
__device__ inline const double *atrous_dual_slope(const DualBlock *, const double *m) { return m; }

// in / next: twelve planes of N = W*H doubles (above).  planes (GUIDED): dual_feature_planes_kernel's 14 planes.  tiles_x: workgroups per row of
// tiles (the grid is one-dimensional: a frame may be taller than 65,535 tiles).  REGION: one more argument, the block table; workgroup b owns the pixels
// at entry b's origin before its far corner (inside the frame), tiles_x is not read.  SLOPE (GUIDED only): one more argument after that, the seven slope planes
template <bool GUIDED, bool LAST, bool REGION = false, class... T>
__global__ __launch_bounds__(kAtrousDualBlockW *kAtrousDualBlockH) void atrous_dual_level_kernel(
    const double *__restrict__ in, double *__restrict__ next, const double *__restrict__ SA, const double *__restrict__ SB, const uint32_t *__restrict__ n_a,
    const uint32_t *__restrict__ n_b, uint32_t W, uint32_t H, uint32_t tiles_x, int64_t step, double k2, double alpha, const double *__restrict__ planes, double kf2,
    double tau, double *__restrict__ out, double *__restrict__ err, T... table) {
	static_assert(sizeof...(T) == (REGION ? 1 : 0) || (GUIDED && sizeof...(T) == (REGION ? 2 : 1)), "the block table, with REGION only, then the slope planes, with GUIDED only");
	constexpr bool SLOPE = sizeof...(T) == (REGION ? 2 : 1);
	[[maybe_unused]] DualBlock e{};
	if constexpr (REGION) e = atrous_dual_table(table...)[blockIdx.x];
	// (REGION is a constant: each conditional below is one of its arms, and the whole-frame instantiations are compiled from the lines they always had)
	const uint32_t bx = REGION ? 0u : blockIdx.x % tiles_x, by = REGION ? 0u : blockIdx.x / tiles_x;
	const int64_t x = REGION ? (int64_t)e.x0 + (threadIdx.x % kAtrousDualBlockW) : (int64_t)bx * kAtrousDualBlockW + (threadIdx.x % kAtrousDualBlockW),
	              y = REGION ? (int64_t)e.y0 + (threadIdx.x / kAtrousDualBlockW) : (int64_t)by * kAtrousDualBlockH + (threadIdx.x / kAtrousDualBlockW);
	if (x >= (REGION ? (int64_t)e.x_end : (int64_t)W) || y >= (REGION ? (int64_t)e.y_end : (int64_t)H)) return;
	const size_t N = (size_t)W * H, pix = (size_t)x + (size_t)y * W;
	const double ap0 = in[pix];
	if (!(ap0 == ap0)) { // not dual-valid: never a tap, so only its mark is kept
		if constexpr (LAST) dual_merged(SA, SB, (double)n_a[pix], (double)n_b[pix], pix, out, err);
		else next[pix] = ap0;
		return;
	}
	// p's state: half A's c and v, half B's c and v
	const double ap1 = in[N + pix], ap2 = in[2 * N + pix], sp0 = in[3 * N + pix], sp1 = in[4 * N + pix], sp2 = in[5 * N + pix];
	const double bp0 = in[6 * N + pix], bp1 = in[7 * N + pix], bp2 = in[8 * N + pix], tp0 = in[9 * N + pix], tp1 = in[10 * N + pix], tp2 = in[11 * N + pix];
	// GUIDED: this pixel's features, their variances and the denominators of Phi_j(p, .), as atrous_level_kernel makes them
	[[maybe_unused]] double fp[kDenoiseFeat], gp[kDenoiseFeat], den[kDenoiseFeat];
	[[maybe_unused]] bool p_fok = false;
	if constexpr (GUIDED) {
#pragma unroll
		for (int j = 0; j < kDenoiseFeat; j++) { // SLOPE: the seven floors first, into den's registers — read beside f and g they cost two VGPRs and a wave per SIMD
			if constexpr (SLOPE) den[j] = atrous_dual_slope(table...)[(size_t)j * N + pix];
		}
#pragma unroll
		for (int j = 0; j < kDenoiseFeat; j++) {
			fp[j] = planes[(size_t)j * N + pix], gp[j] = planes[(size_t)(kDenoiseFeat + j) * N + pix];
			if constexpr (SLOPE) den[j] = feature_den(fp[j], gp[j], j, kf2, tau, den[j]);
			else den[j] = feature_den(fp[j], gp[j], j, kf2, tau);
		}
		p_fok = fp[0] == fp[0];
	}
	// half A's sums under w_B (a, s, wsa), half B's under w_A (b, t, wsb)
	double a0 = 0.0, a1 = 0.0, a2 = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, wsa = 0.0;
	double b0 = 0.0, b1 = 0.0, b2 = 0.0, t0 = 0.0, t1 = 0.0, t2 = 0.0, wsb = 0.0;
	for (int j = -2; j <= 2; j++) {
		const int64_t qy = y + step * j;
		if (qy < 0 || qy >= (int64_t)H) continue;
		for (int i = -2; i <= 2; i++) {
			const int64_t qx = x + step * i;
			if (qx < 0 || qx >= (int64_t)W) continue;
			const size_t q = (size_t)qx + (size_t)qy * W;
			const double aq0 = in[q];
			if (!(aq0 == aq0)) continue;
			const double aq1 = in[N + q], aq2 = in[2 * N + q], sq0 = in[3 * N + q], sq1 = in[4 * N + q], sq2 = in[5 * N + q];
			const double bq0 = in[6 * N + q], bq1 = in[7 * N + q], bq2 = in[8 * N + q], tq0 = in[9 * N + q], tq1 = in[10 * N + q], tq2 = in[11 * N + q];
			const double DA = ((denoise_term(ap0, aq0, sp0, sq0, k2, alpha) + denoise_term(ap1, aq1, sp1, sq1, k2, alpha)) + denoise_term(ap2, aq2, sp2, sq2, k2, alpha)) / 3.0;
			const double DB = ((denoise_term(bp0, bq0, tp0, tq0, k2, alpha) + denoise_term(bp1, bq1, tp1, tq1, k2, alpha)) + denoise_term(bp2, bq2, tp2, tq2, k2, alpha)) / 3.0;
			double wA = exp(-(DA > 0.0 ? DA : 0.0)), wB = exp(-(DB > 0.0 ? DB : 0.0));
			if constexpr (GUIDED) {
				if (p_fok) {
					const double fq0 = planes[q];
					if (fq0 == fq0) { // q is feature-valid too
						double Df = 0.0;
#pragma unroll
						for (int c = 0; c < kDenoiseFeat; c++) {
							const double fq = c == 0 ? fq0 : planes[(size_t)c * N + q], gq = planes[(size_t)(kDenoiseFeat + c) * N + q];
							const double phi = feature_phi(fp[c], gp[c], den[c], fq, gq);
							if (phi > Df) Df = phi; // (a NaN is skipped by the comparison)
						}
						const double wf = exp(-Df); // once, for both passes
						if (wf < wA) wA = wf;
						if (wf < wB) wB = wf;
					}
				}
			}
			const double h = atrous_h5(i) * atrous_h5(j);
			const double hwB = h * wB, hwB2 = hwB * hwB, hwA = h * wA, hwA2 = hwA * hwA;
			a0 = a0 + hwB * aq0, a1 = a1 + hwB * aq1, a2 = a2 + hwB * aq2;
			s0 = s0 + hwB2 * sq0, s1 = s1 + hwB2 * sq1, s2 = s2 + hwB2 * sq2;
			wsa = wsa + hwB;
			b0 = b0 + hwA * bq0, b1 = b1 + hwA * bq1, b2 = b2 + hwA * bq2;
			t0 = t0 + hwA2 * tq0, t1 = t1 + hwA2 * tq1, t2 = t2 + hwA2 * tq2;
			wsb = wsb + hwA;
		}
	}
	if constexpr (LAST) {
		const double fa[3] = {a0 / wsa, a1 / wsa, a2 / wsa}, fb[3] = {b0 / wsb, b1 / wsb, b2 / wsb};
		dual_combine(fa, fb, (double)n_a[pix], (double)n_b[pix], pix, out, err);
	} else {
		const double wa2 = wsa * wsa, wb2 = wsb * wsb;
		next[pix] = a0 / wsa, next[N + pix] = a1 / wsa, next[2 * N + pix] = a2 / wsa;
		next[3 * N + pix] = s0 / wa2, next[4 * N + pix] = s1 / wa2, next[5 * N + pix] = s2 / wa2;
		next[6 * N + pix] = b0 / wsb, next[7 * N + pix] = b1 / wsb, next[8 * N + pix] = b2 / wsb;
		next[9 * N + pix] = t0 / wb2, next[10 * N + pix] = t1 / wb2, next[11 * N + pix] = t2 / wb2;
	}
}

hipError_t launch_denoise_atrous_dual(hipStream_t stream, const DenoiseInput &in, const DenoiseWeights &w, uint32_t levels, uint32_t *n_img, double *state,
                                      uint32_t *n_f_img, double *feat_planes, double *slope_planes, double *out, double *err) {
	if (levels > kAtrousMaxLevels) return hipErrorInvalidValue;
	const bool guided = in.feat != nullptr && levels != 0u, sloped = guided && w.slope > 0.0;
	if (guided && (in.feat_sq == nullptr || n_f_img == nullptr || feat_planes == nullptr || (in.n_rects && in.counts_f == nullptr))) return hipErrorInvalidValue;
	if (sloped && slope_planes == nullptr) return hipErrorInvalidValue;
	const double *accum_a = in.accum_a, *accum_b = in.accum_b;
	const uint32_t W = in.W, H = in.H;
	const double alpha = w.alpha, tau = w.tau;
	const size_t N = (size_t)W * H;
	const uint64_t blocks_1d = ((uint64_t)N + 255u) / 256u;
	const uint32_t tiles_x = (W + kAtrousDualBlockW - 1u) / kAtrousDualBlockW;
	const uint64_t tiles = (uint64_t)tiles_x * ((H + kAtrousDualBlockH - 1u) / kAtrousDualBlockH);
	if (blocks_1d > 0x7FFFFFFFull || tiles > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
	DenoiseInput pre = in; // (levels = 0 reads no feature)
	if (!guided) pre.feat = pre.feat_sq = nullptr;
	hipError_t e = launch_dual_planes(stream, pre, n_img, state, n_f_img, feat_planes);
	if (e != hipSuccess) return e;
	const uint32_t *n_a = n_img, *n_b = n_img + N;
	if (levels == 0u) {
		hipLaunchKernelGGL(atrous_dual_mean_kernel, dim3((uint32_t)blocks_1d), dim3(256), 0, stream, state, accum_a, accum_b, n_a, n_b, N, out, err);
		return hipGetLastError();
	}
	const double k2 = w.k * w.k, kf2 = w.k_f * w.k_f;
	const dim3 grid((uint32_t)tiles), block(kAtrousDualBlockW * kAtrousDualBlockH);
	if (sloped && (e = launch_feature_slope(stream, feat_planes, W, H, w.slope, slope_planes)) != hipSuccess) return e; // (once: the features are every level's)
	const double *m = slope_planes;
	double *set[2] = {state, state + 12u * N};
	for (uint32_t l = 0; l < levels; l++) {
		const double *in = set[l & 1u];
		double *next = set[(l + 1u) & 1u];
		const int64_t step = (int64_t)1 << l;
		const bool last = l + 1u == levels;
		if (sloped) {
			if (last) hipLaunchKernelGGL((atrous_dual_level_kernel<true, true, false, const double *>), grid, block, 0, stream, in, next, accum_a, accum_b, n_a, n_b, W, H, tiles_x, step, k2, alpha, feat_planes, kf2, tau, out, err, m);
			else hipLaunchKernelGGL((atrous_dual_level_kernel<true, false, false, const double *>), grid, block, 0, stream, in, next, accum_a, accum_b, n_a, n_b, W, H, tiles_x, step, k2, alpha, feat_planes, kf2, tau, out, err, m);
		} else if (guided) {
			if (last) hipLaunchKernelGGL((atrous_dual_level_kernel<true, true>), grid, block, 0, stream, in, next, accum_a, accum_b, n_a, n_b, W, H, tiles_x, step, k2, alpha, feat_planes, kf2, tau, out, err);
			else hipLaunchKernelGGL((atrous_dual_level_kernel<true, false>), grid, block, 0, stream, in, next, accum_a, accum_b, n_a, n_b, W, H, tiles_x, step, k2, alpha, feat_planes, kf2, tau, out, err);
		} else {
			if (last) hipLaunchKernelGGL((atrous_dual_level_kernel<false, true>), grid, block, 0, stream, in, next, accum_a, accum_b, n_a, n_b, W, H, tiles_x, step, k2, alpha, feat_planes, kf2, tau, out, err);
			else hipLaunchKernelGGL((atrous_dual_level_kernel<false, false>), grid, block, 0, stream, in, next, accum_a, accum_b, n_a, n_b, W, H, tiles_x, step, k2, alpha, feat_planes, kf2, tau, out, err);
		}
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	return hipSuccess;
}

// One level of the region call over `n_blocks` entries of `table`; m (at most one, GUIDED only): the slope planes
template <bool GUIDED, bool LAST, class... M>
static hipError_t launch_atrous_dual_region_level(hipStream_t stream, const DualBlock *table, uint32_t n_blocks, const double *in, double *next, const double *SA,
                                                  const double *SB, const uint32_t *n_a, const uint32_t *n_b, uint32_t W, uint32_t H, int64_t step, double k2, double alpha,
                                                  const double *fplanes, double kf2, double tau, double *out, double *err, M... m) {
	if constexpr (sizeof...(M) != 0)
		hipLaunchKernelGGL((atrous_dual_level_kernel<GUIDED, LAST, true, const DualBlock *, const double *>), dim3(n_blocks), dim3(kAtrousDualBlockW * kAtrousDualBlockH), 0, stream,
		                   in, next, SA, SB, n_a, n_b, W, H, 0u, step, k2, alpha, fplanes, kf2, tau, out, err, table, m...);
	else hipLaunchKernelGGL((atrous_dual_level_kernel<GUIDED, LAST, true, const DualBlock *>), dim3(n_blocks), dim3(kAtrousDualBlockW * kAtrousDualBlockH), 0, stream, in, next, SA,
	                   SB, n_a, n_b, W, H, 0u, step, k2, alpha, fplanes, kf2, tau, out, err, table);
	return hipGetLastError();
}

hipError_t launch_denoise_atrous_dual_region(hipStream_t stream, const DenoiseInput &in, const DenoiseWeights &w, uint32_t levels, uint32_t *n_img, double *state,
                                             uint32_t *n_f_img, double *feat_planes, double *slope_planes, const DualBlock *table, const uint32_t *table_first,
                                             const uint32_t *table_count, double *out, double *err) {
	if (levels > kAtrousMaxLevels || table == nullptr || table_first == nullptr || table_count == nullptr) return hipErrorInvalidValue;
	const bool guided = in.feat != nullptr && levels != 0u, sloped = guided && w.slope > 0.0;
	if (guided && (in.feat_sq == nullptr || n_f_img == nullptr || feat_planes == nullptr || (in.n_rects && in.counts_f == nullptr))) return hipErrorInvalidValue;
	if (sloped && slope_planes == nullptr) return hipErrorInvalidValue;
	const double *accum_a = in.accum_a, *accum_sq_a = in.accum_sq_a, *accum_b = in.accum_b, *accum_sq_b = in.accum_sq_b;
	const uint32_t W = in.W, H = in.H;
	const double alpha = w.alpha, tau = w.tau;
	for (uint32_t i = 0; i <= levels; i++)
		if (table_count[i] == 0u || table_count[i] > 0x7FFFFFFFu) return hipErrorInvalidConfiguration; // (a region with pixels needs every table; the caller returns before an empty one)
	const size_t N = (size_t)W * H;
	uint32_t *n_a = n_img, *n_b = n_img + N;
	// the count images: the whole frame's, as launch_dual_planes makes them (a memset and the painting of the rects)
	hipError_t e = hipMemsetAsync(n_img, 0, 2u * N * sizeof(uint32_t), stream);
	if (e != hipSuccess) return e;
	if (guided && (e = hipMemsetAsync(n_f_img, 0, N * sizeof(uint32_t), stream)) != hipSuccess) return e;
	if (in.n_rects) {
		hipLaunchKernelGGL(atrous_dual_count_image_kernel, dim3(in.n_rects, in.count_image_columns), dim3(256), 0, stream, in.rects, in.counts_a, in.counts_b,
		                   guided ? in.counts_f : nullptr, W, n_a, n_b, guided ? n_f_img : nullptr);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	const dim3 block(kAtrousDualBlockW * kAtrousDualBlockH);
	if (guided) hipLaunchKernelGGL(atrous_dual_planes_region_kernel<true>, dim3(table_count[0]), block, 0, stream, accum_a, accum_sq_a, accum_b, accum_sq_b, in.feat, in.feat_sq, n_a, n_b, n_f_img, table + table_first[0], W, N, state, feat_planes);
	else hipLaunchKernelGGL(atrous_dual_planes_region_kernel<false>, dim3(table_count[0]), block, 0, stream, accum_a, accum_sq_a, accum_b, accum_sq_b, nullptr, nullptr, n_a, n_b, nullptr, table + table_first[0], W, N, state, nullptr);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (levels == 0u) { // (table 0 is the region's own then)
		hipLaunchKernelGGL(atrous_dual_mean_region_kernel, dim3(table_count[0]), block, 0, stream, state, accum_a, accum_b, n_a, n_b, table + table_first[0], W, N, out, err);
		return hipGetLastError();
	}
	const double k2 = w.k * w.k, kf2 = w.k_f * w.k_f;
	const double *m = slope_planes;
	if (sloped) { // on level 0's table: every later level's pixels lie in it, and table 0, made above, reaches two pixels further
		hipLaunchKernelGGL(atrous_dual_slope_region_kernel, dim3(table_count[1]), block, 0, stream, feat_planes, table + table_first[1], W, H, N, w.slope * w.slope, slope_planes);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	double *set[2] = {state, state + 12u * N};
	for (uint32_t l = 0; l < levels; l++) {
		const double *in = set[l & 1u];
		double *next = set[(l + 1u) & 1u];
		const int64_t step = (int64_t)1 << l;
		const bool last = l + 1u == levels;
		const DualBlock *t = table + table_first[l + 1u];
		const uint32_t nb = table_count[l + 1u];
		if (sloped) e = last ? launch_atrous_dual_region_level<true, true>(stream, t, nb, in, next, accum_a, accum_b, n_a, n_b, W, H, step, k2, alpha, feat_planes, kf2, tau, out, err, m)
			                 : launch_atrous_dual_region_level<true, false>(stream, t, nb, in, next, accum_a, accum_b, n_a, n_b, W, H, step, k2, alpha, feat_planes, kf2, tau, out, err, m);
		else if (guided) e = last ? launch_atrous_dual_region_level<true, true>(stream, t, nb, in, next, accum_a, accum_b, n_a, n_b, W, H, step, k2, alpha, feat_planes, kf2, tau, out, err)
			                 : launch_atrous_dual_region_level<true, false>(stream, t, nb, in, next, accum_a, accum_b, n_a, n_b, W, H, step, k2, alpha, feat_planes, kf2, tau, out, err);
		else e = last ? launch_atrous_dual_region_level<false, true>(stream, t, nb, in, next, accum_a, accum_b, n_a, n_b, W, H, step, k2, alpha, feat_planes, kf2, tau, out, err)
			          : launch_atrous_dual_region_level<false, false>(stream, t, nb, in, next, accum_a, accum_b, n_a, n_b, W, H, step, k2, alpha, feat_planes, kf2, tau, out, err);
		if (e != hipSuccess) return e;
	}
	return hipSuccess;
}

} // namespace rmd
