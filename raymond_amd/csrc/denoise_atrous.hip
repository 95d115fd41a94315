// Edge-avoiding a-trous wavelet filter over a rendered frame (rmd_denoise_atrous; include/raymond_hip.h states the definition, DESIGN.md
// section 17 the structure and its cost).  A translation unit of its own: no other unit's code objects change.
//
// atrous_prologue_kernel        — c^0 = u and v^0 = v per pixel from S, Q and the count image (denoise.hip: launch_denoise_planes), into six
//                                 planar W*H images; a pixel that is not valid keeps a NaN in plane 0 (the unit's habit: denoise.hip's apron).
// atrous_level_kernel<G, LAST>  — one level: one thread per pixel, 64 x 4 pixels per workgroup (a wave is 64 neighbouring pixels of one row), the
//                                 25 taps at step s read straight from the planar images in global memory: every tap's load is one contiguous
//                                 row segment per wave, and the taps of a 5 x 5 stencil are reread by the neighbouring waves out of L2.  No LDS:
//                                 an apron pays for itself only at steps 1 and 2, and a second shape for those two levels was not taken
//                                 (DESIGN.md section 17).  p's c, v — and with G (guided) its seven f, g and denominators — live in registers.
//                                 LAST = false writes c^{l+1}, v^{l+1} into the other set of six planes; LAST = true writes the interleaved
//                                 out_dev, and S / n for a pixel that is not valid.
// atrous_mean_kernel            — levels = 0: out = S / n for every pixel.
// SLOPE (rmd_denoise_atrous_slope at slope > 0): atrous_level_kernel<true, LAST, const double *> takes one more trailing argument, the
//                                 seven planes m that denoise.hip's feature_slope_kernel makes of the f planes (launch_feature_slope), and reads p's
//                                 seven m once, where the denominators are made: the same m at every level.  The instantiations without it keep their
//                                 arguments and their instructions.
// The count image and the 14 feature planes are denoise.hip's, the per-pixel arithmetic denoise_device.hpp's.  f64 throughout, built with -ffp-contract=off like the rest of the library.
#include <hip/hip_runtime.h>

#include "denoise_device.hpp"

namespace rmd {

constexpr int kAtrousBlockW = 64, kAtrousBlockH = 4;

__global__ __launch_bounds__(256) void atrous_prologue_kernel(const double *__restrict__ S, const double *__restrict__ Q, const uint32_t *__restrict__ n_img,
                                                              size_t N, double *__restrict__ cv) {
	const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= N) return;
	double u[3], v[3];
	const bool valid = moments_pixel(S, Q, i, n_img[i], u, v);
	cv[i] = valid ? u[0] : __builtin_nan(""), cv[N + i] = u[1], cv[2 * N + i] = u[2];
	cv[3 * N + i] = v[0], cv[4 * N + i] = v[1], cv[5 * N + i] = v[2];
}

__global__ __launch_bounds__(256) void atrous_mean_kernel(const double *__restrict__ S, const uint32_t *__restrict__ n_img, size_t N, double *__restrict__ out) {
	const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= N) return;
	const double nd = (double)n_img[i];
	out[i * 3 + 0] = S[i * 3 + 0] / nd, out[i * 3 + 1] = S[i * 3 + 1] / nd, out[i * 3 + 2] = S[i * 3 + 2] / nd;
}

// in / next: six planes of N = W*H doubles, c of channel 0..2 then v of channel 0..2.  planes (GUIDED): feature_planes_kernel's 14 planes.
// tiles_x: workgroups per row of tiles (the grid is one-dimensional: a frame may be taller than 65,535 tiles)
// m (GUIDED only, at most one): feature_slope_kernel's seven planes, the floors under the denominators
__device__ inline const double *atrous_slope_planes(const double *m) { return m; }
template <bool GUIDED, bool LAST, class... M>
__global__ __launch_bounds__(kAtrousBlockW *kAtrousBlockH) void atrous_level_kernel(const double *__restrict__ in, double *__restrict__ next,
                                                                                    const double *__restrict__ S, const uint32_t *__restrict__ n_img, uint32_t W,
                                                                                    uint32_t H, uint32_t tiles_x, int64_t step, double k2, double alpha,
                                                                                    const double *__restrict__ planes, double kf2, double tau,
                                                                                    double *__restrict__ out, M... m) {
	static_assert(sizeof...(M) <= (GUIDED ? 1 : 0), "the slope planes, with GUIDED only");
	const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
	const int64_t x = (int64_t)bx * kAtrousBlockW + (threadIdx.x % kAtrousBlockW), y = (int64_t)by * kAtrousBlockH + (threadIdx.x / kAtrousBlockW);
	if (x >= (int64_t)W || y >= (int64_t)H) return;
	const size_t N = (size_t)W * H, pix = (size_t)x + (size_t)y * W;
	const double cp0 = in[pix];
	if (!(cp0 == cp0)) { // not valid: never a tap, so only its mark is kept; the last level writes the mean exactly as IEEE gives it
		if constexpr (LAST) {
			const double nd = (double)n_img[pix];
			out[pix * 3 + 0] = S[pix * 3 + 0] / nd, out[pix * 3 + 1] = S[pix * 3 + 1] / nd, out[pix * 3 + 2] = S[pix * 3 + 2] / nd;
		} else {
			next[pix] = cp0;
		}
		return;
	}
	const double cp1 = in[N + pix], cp2 = in[2 * N + pix], vp0 = in[3 * N + pix], vp1 = in[4 * N + pix], vp2 = in[5 * N + pix];
	// GUIDED: this pixel's features, their variances and the denominators of Phi_j(p, .), as denoise_kernel<TW, DenoiseGuide> makes them
	[[maybe_unused]] double fp[kDenoiseFeat], gp[kDenoiseFeat], den[kDenoiseFeat];
	[[maybe_unused]] bool p_fok = false;
	if constexpr (GUIDED) {
#pragma unroll
		for (int j = 0; j < kDenoiseFeat; j++) { // the slope form: the seven floors first, into den's registers (atrous_dual_level_kernel's order)
			if constexpr (sizeof...(M) != 0) den[j] = atrous_slope_planes(m...)[(size_t)j * N + pix];
		}
#pragma unroll
		for (int j = 0; j < kDenoiseFeat; j++) {
			fp[j] = planes[(size_t)j * N + pix], gp[j] = planes[(size_t)(kDenoiseFeat + j) * N + pix];
			if constexpr (sizeof...(M) != 0) den[j] = feature_den(fp[j], gp[j], j, kf2, tau, den[j]);
			else den[j] = feature_den(fp[j], gp[j], j, kf2, tau);
		}
		p_fok = fp[0] == fp[0];
	}
	double a0 = 0.0, a1 = 0.0, a2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, wsum = 0.0;
	for (int j = -2; j <= 2; j++) {
		const int64_t qy = y + step * j;
		if (qy < 0 || qy >= (int64_t)H) continue;
		for (int i = -2; i <= 2; i++) {
			const int64_t qx = x + step * i;
			if (qx < 0 || qx >= (int64_t)W) continue;
			const size_t q = (size_t)qx + (size_t)qy * W;
			const double cq0 = in[q];
			if (!(cq0 == cq0)) continue;
			const double cq1 = in[N + q], cq2 = in[2 * N + q], vq0 = in[3 * N + q], vq1 = in[4 * N + q], vq2 = in[5 * N + q];
			const double D = ((denoise_term(cp0, cq0, vp0, vq0, k2, alpha) + denoise_term(cp1, cq1, vp1, vq1, k2, alpha)) + denoise_term(cp2, cq2, vp2, vq2, k2, alpha)) / 3.0;
			double w = exp(-(D > 0.0 ? D : 0.0));
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
						const double wf = exp(-Df);
						if (wf < w) w = wf;
					}
				}
			}
			const double hw = (atrous_h5(i) * atrous_h5(j)) * w, hw2 = hw * hw;
			a0 = a0 + hw * cq0, a1 = a1 + hw * cq1, a2 = a2 + hw * cq2;
			b0 = b0 + hw2 * vq0, b1 = b1 + hw2 * vq1, b2 = b2 + hw2 * vq2;
			wsum = wsum + hw;
		}
	}
	if constexpr (LAST) {
		out[pix * 3 + 0] = a0 / wsum, out[pix * 3 + 1] = a1 / wsum, out[pix * 3 + 2] = a2 / wsum;
	} else {
		const double w2 = wsum * wsum;
		next[pix] = a0 / wsum, next[N + pix] = a1 / wsum, next[2 * N + pix] = a2 / wsum;
		next[3 * N + pix] = b0 / w2, next[4 * N + pix] = b1 / w2, next[5 * N + pix] = b2 / w2;
	}
}

hipError_t launch_denoise_atrous(hipStream_t stream, const DenoiseInput &in, const DenoiseWeights &w, uint32_t levels, uint32_t *n_img, double *cv, double *feat_planes,
                                 double *slope_planes, double *out) {
	if (levels > kAtrousMaxLevels) return hipErrorInvalidValue;
	const bool guided = in.feat != nullptr && levels != 0u, sloped = guided && w.slope > 0.0;
	if (in.feat != nullptr && (in.feat_sq == nullptr || feat_planes == nullptr)) return hipErrorInvalidValue;
	if (sloped && slope_planes == nullptr) return hipErrorInvalidValue;
	DenoiseInput pre = in; // (levels = 0 reads no feature)
	if (!guided) pre.feat = pre.feat_sq = nullptr;
	hipError_t e = launch_denoise_planes(stream, pre, n_img, feat_planes);
	if (e != hipSuccess) return e;
	const double *accum = in.accum_a, *accum_sq = in.accum_sq_a;
	const uint32_t W = in.W, H = in.H;
	const double alpha = w.alpha, tau = w.tau;
	const size_t N = (size_t)W * H;
	const uint64_t blocks_1d = ((uint64_t)N + 255u) / 256u;
	const uint32_t tiles_x = (W + kAtrousBlockW - 1u) / kAtrousBlockW;
	const uint64_t tiles = (uint64_t)tiles_x * ((H + kAtrousBlockH - 1u) / kAtrousBlockH);
	if (blocks_1d > 0x7FFFFFFFull || tiles > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
	if (levels == 0u) {
		hipLaunchKernelGGL(atrous_mean_kernel, dim3((uint32_t)blocks_1d), dim3(256), 0, stream, accum, n_img, N, out);
		return hipGetLastError();
	}
	hipLaunchKernelGGL(atrous_prologue_kernel, dim3((uint32_t)blocks_1d), dim3(256), 0, stream, accum, accum_sq, n_img, N, cv);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (sloped && (e = launch_feature_slope(stream, feat_planes, W, H, w.slope, slope_planes)) != hipSuccess) return e; // (once: the features are every level's)
	const double *m = slope_planes;
	const double k2 = w.k * w.k, kf2 = w.k_f * w.k_f;
	const dim3 grid((uint32_t)tiles), block(kAtrousBlockW * kAtrousBlockH);
	double *set[2] = {cv, cv + 6u * N};
	for (uint32_t l = 0; l < levels; l++) {
		const double *in = set[l & 1u];
		double *next = set[(l + 1u) & 1u];
		const int64_t step = (int64_t)1 << l;
		const bool last = l + 1u == levels;
		if (sloped) {
			if (last) hipLaunchKernelGGL((atrous_level_kernel<true, true, const double *>), grid, block, 0, stream, in, next, accum, n_img, W, H, tiles_x, step, k2, alpha, feat_planes, kf2, tau, out, m);
			else hipLaunchKernelGGL((atrous_level_kernel<true, false, const double *>), grid, block, 0, stream, in, next, accum, n_img, W, H, tiles_x, step, k2, alpha, feat_planes, kf2, tau, out, m);
		} else if (guided) {
			if (last) hipLaunchKernelGGL((atrous_level_kernel<true, true>), grid, block, 0, stream, in, next, accum, n_img, W, H, tiles_x, step, k2, alpha, feat_planes, kf2, tau, out);
			else hipLaunchKernelGGL((atrous_level_kernel<true, false>), grid, block, 0, stream, in, next, accum, n_img, W, H, tiles_x, step, k2, alpha, feat_planes, kf2, tau, out);
		} else {
			if (last) hipLaunchKernelGGL((atrous_level_kernel<false, true>), grid, block, 0, stream, in, next, accum, n_img, W, H, tiles_x, step, k2, alpha, feat_planes, kf2, tau, out);
			else hipLaunchKernelGGL((atrous_level_kernel<false, false>), grid, block, 0, stream, in, next, accum, n_img, W, H, tiles_x, step, k2, alpha, feat_planes, kf2, tau, out);
		}
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	return hipSuccess;
}

} // namespace rmd
