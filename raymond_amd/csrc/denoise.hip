// Variance-guided non-local means over a rendered frame (rmd_denoise; include/raymond_hip.h states the definition, DESIGN.md section 11 the
// structure and its cost).  A translation unit of its own: the render kernels' code objects do not change.  The per-pixel arithmetic — the term, the
// moments, the feature weight's pieces — is denoise_device.hpp's, shared with the other three denoise units.
//
// count_image_kernel — the rects' sample counts expanded into one count per pixel (0 where no rect lies): a column of workgroups per rect.
// denoise_kernel<TW> — one TW x 16 output tile per workgroup of TW * 16 threads, one output pixel per thread.  TW = 32 (8 waves: two per SIMD,
//                      and less apron per output pixel) when its LDS fits, else TW = 24 (r = 12 with f = 4):
//   1. the apron (tile +- (r + f), clamped to the frame) is staged into LDS as the per-pixel mean u and the variance of the mean v, 48 B a
//      pixel in six planes; an invalid pixel keeps a NaN in its u of channel 0;
//   2. for each neighbour offset d, in raster order: the term image T_d(a) = sum_c term_c(clamp(a), clamp(a + d)) and its taken-count at every
//      position a of tile +- f (each thread holds its positions' own u and v in registers for the whole loop), then the row sums over the
//      patch's 2f+1 columns, then each thread's column sum over 2f+1 rows: D(p, p + d) without recomputing a patch per pixel.  Each window
//      is summed directly: a running sum that subtracts would lose the small terms beside a (du)^2 / eps one;
//   3. w = exp(-max(0, D)) and w * u_q are accumulated in registers.
// GUIDED (rmd_denoise_guided; denoise_kernel<TW, DenoiseGuide>, instantiations of their own so that the unguided ones are compiled exactly as
// without the feature): step 3 also makes the feature weight w_f of the pixel pair and takes min(w, w_f).  p's seven f, g and denominators live in registers;
// q's f and g are read per offset straight from planar images in global memory (feature_planes_kernel writes them: 14 planes of W*H doubles, a
// pixel that is not feature-valid keeps a NaN in its f of channel 0) — neighbouring lanes read neighbouring doubles and consecutive offsets shift
// by one pixel, so these are cache hits; f64 planes for the apron do not fit in LDS beside the colour planes.
// SLOPE (rmd_denoise_guided_slope at slope > 0): feature_slope_kernel makes seven more planes, the slope floors m of the seven f
// planes, and denoise_kernel<TW, DenoiseSlope> — instantiations of their own again — reads p's seven m once, where the denominators are made.  At slope 0
// neither is launched.
// f64 throughout, built with -ffp-contract=off like the rest of the library.
#include <hip/hip_runtime.h>

#include "denoise_device.hpp"

namespace rmd {

__global__ __launch_bounds__(256) void count_image_kernel(const rmd_tile_rect *__restrict__ rects, const uint32_t *__restrict__ counts, uint32_t W,
                                                          uint32_t *__restrict__ n_img) {
	const rmd_tile_rect r = rects[blockIdx.x];
	const uint32_t n = counts[blockIdx.x];
	const uint64_t n_px = (uint64_t)r.width * r.height;
	for (uint64_t i = (uint64_t)blockIdx.y * 256u + threadIdx.x; i < n_px; i += (uint64_t)gridDim.y * 256u) n_img[rect_pixel(r, i, W)] = n;
}

// Per pixel: feature_planes_pixel's fourteen planes (N = W*H doubles each), seeded with the pixel's own validity: n >= 2 and finite S, Q.
__global__ __launch_bounds__(256) void feature_planes_kernel(const double *__restrict__ S, const double *__restrict__ Q, const double *__restrict__ F,
                                                             const double *__restrict__ G, const uint32_t *__restrict__ n_img, size_t N,
                                                             double *__restrict__ planes) {
	const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= N) return;
	const uint32_t n = n_img[i];
	double u[3], v[3];
	feature_planes_pixel(F, G, i, n, moments_pixel(S, Q, i, n, u, v), N, planes);
}

// The slope floors of rmd_denoise_guided_slope and of the dual _slope calls (denoise_dual.hip's launchers and the whole-frame a-trous ones call launch_feature_slope too): feature_slope_pixel's
// seven planes m from the seven planar f that feature_planes_kernel / dual_feature_planes_kernel have written.  Whole-frame in every form.  Consecutive
// lanes hold consecutive pixels of a row, so each of the five reads per channel is coalesced
__global__ __launch_bounds__(256) void feature_slope_kernel(const double *__restrict__ fplanes, uint32_t W, uint32_t H, double s2, double *__restrict__ mplanes) {
	const size_t N = (size_t)W * H, i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= N) return;
	feature_slope_pixel(fplanes, i, (uint32_t)(i % W), (uint32_t)(i / W), W, H, N, s2, mplanes);
}
hipError_t launch_feature_slope(hipStream_t stream, const double *feat_planes, uint32_t W, uint32_t H, double slope, double *slope_planes) {
	if (feat_planes == nullptr || slope_planes == nullptr) return hipErrorInvalidValue;
	const size_t N = (size_t)W * H;
	hipLaunchKernelGGL(feature_slope_kernel, dim3((uint32_t)((N + 255u) / 256u)), dim3(256), 0, stream, feat_planes, W, H, slope * slope, slope_planes);
	return hipGetLastError();
}

// the guided kernel's extra arguments: the planar f and g images, k_f^2 and tau
struct DenoiseGuide {
	const double *planes;
	double kf2, tau;
};
// ... and with the slope floors (rmd_denoise_guided_slope at slope > 0): feature_slope_kernel's seven planes m
struct DenoiseSlope : DenoiseGuide {
	const double *m;
};
// GUIDED is the presence of a DenoiseGuide argument: denoise_kernel<TW> (no such argument) keeps the signature and the code it had before the
// guided filter existed, denoise_kernel<TW, DenoiseGuide> is the guided instantiation.  SLOPE: the argument is a DenoiseSlope — an instantiation of its
// own again (denoise_kernel<TW, DenoiseSlope>), which reads p's seven m once, where den is made; the per-pair loop is the guided one's.
template <int TW, class... G>
__global__ __launch_bounds__(TW * 16) void denoise_kernel(const double *__restrict__ S, const double *__restrict__ Q, const uint32_t *__restrict__ n_img,
                                                          uint32_t W, uint32_t H, int r, int f, double k2, double alpha, double *__restrict__ out, G... guide) {
	constexpr bool GUIDED = sizeof...(G) != 0;
	static_assert(sizeof...(G) <= 1, "at most one DenoiseGuide");
	[[maybe_unused]] const double *planes = nullptr;
	[[maybe_unused]] double kf2 = 0.0, tau = 0.0;
	constexpr bool SLOPE = (__is_same(G, DenoiseSlope) || ...);
	[[maybe_unused]] const double *mplanes = nullptr;
	if constexpr (GUIDED) {
		const DenoiseGuide gd = (guide, ...);
		planes = gd.planes, kf2 = gd.kf2, tau = gd.tau;
		if constexpr (SLOPE) mplanes = (guide, ...).m;
	}
	extern __shared__ double lds[];
	constexpr int TH = (int)kDenoiseTile, NT = TW * TH;
	const int R = r + f, AW = TW + 2 * R, AA = AW * (TH + 2 * R), PW = TW + 2 * f, PP = PW * (TH + 2 * f);
	double *U = lds, *V = lds + 3 * AA;           // planes c * AA + (apron row * AW + apron column)
	double *T = lds + 6 * AA, *Hs = T + PP;        // the term image (TH + 2f rows of PW) and its row sums (TH + 2f rows of TW)
	uint32_t *Tc = reinterpret_cast<uint32_t *>(Hs + (TH + 2 * f) * TW), *Hc = Tc + PP;
	const int64_t x0 = (int64_t)blockIdx.x * TW, y0 = (int64_t)blockIdx.y * TH;
	const int tid = threadIdx.x;

	for (int i = tid; i < AA; i += NT) {
		const int ly = i / AW, lx = i - ly * AW;
		const int64_t gx = min(max(x0 - R + lx, (int64_t)0), (int64_t)W - 1), gy = min(max(y0 - R + ly, (int64_t)0), (int64_t)H - 1);
		const size_t pix = (size_t)gx + (size_t)gy * W;
		const uint32_t n = n_img[pix];
		const double nd = (double)n;
		bool valid = n >= 2u;
		double u[3], v[3];
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const double s = S[pix * 3 + c], q = Q[pix * 3 + c];
			valid = valid && __builtin_fabs(s) < __builtin_inf() && __builtin_fabs(q) < __builtin_inf(); // denoise_finite of both, written out: through the call this kernel's instructions change
			denoise_moments(s, q, nd, u[c], v[c]);
		}
		U[i] = valid ? u[0] : __builtin_nan(""), U[AA + i] = u[1], U[2 * AA + i] = u[2];
		V[i] = v[0], V[AA + i] = v[1], V[2 * AA + i] = v[2];
	}
	__syncthreads();

	// this thread's term-image positions (at most 3: PP <= (TW + 8) * 24 <= 3 * TW * 16) and their own u, v
	constexpr int kSlots = 3;
	int ia[kSlots];
	bool oka[kSlots];
	double ua[kSlots][3], va[kSlots][3];
#pragma unroll
	for (int s = 0; s < kSlots; s++) {
		const int j = tid + NT * s;
		const int ty = j / PW, tx = j - ty * PW;
		ia[s] = j < PP ? (ty + r) * AW + (tx + r) : 0;
#pragma unroll
		for (int c = 0; c < 3; c++) ua[s][c] = U[c * AA + ia[s]], va[s][c] = V[c * AA + ia[s]];
		oka[s] = j < PP && ua[s][0] == ua[s][0];
	}

	// this thread's output pixel; the offsets that keep q = p + d inside the frame
	const int px = tid % TW, py = tid / TW;
	const int64_t gx = x0 + px, gy = y0 + py;
	const bool inside = gx < (int64_t)W && gy < (int64_t)H;
	const int ip = (py + R) * AW + (px + R);
	const bool p_ok = inside && U[ip] == U[ip];
	const int dx_lo = (int)max((int64_t)-r, -gx), dx_hi = (int)min((int64_t)r, (int64_t)W - 1 - gx);
	const int dy_lo = (int)max((int64_t)-r, -gy), dy_hi = (int)min((int64_t)r, (int64_t)H - 1 - gy);
	double acc0 = -0.0, acc1 = -0.0, acc2 = -0.0, wsum = -0.0; // -0.0 + x == x for every x, so r = 0 gives S / n bit for bit
	// GUIDED: this pixel's features, their variances and the denominators of Phi_j(p, .)
	[[maybe_unused]] double fp[kDenoiseFeat], gp[kDenoiseFeat], den[kDenoiseFeat];
	[[maybe_unused]] bool p_fok = false;
	[[maybe_unused]] const size_t N = (size_t)W * H;
	[[maybe_unused]] const size_t pixp = inside ? (size_t)gx + (size_t)gy * W : 0;
	if constexpr (GUIDED) {
#pragma unroll
		for (int j = 0; j < kDenoiseFeat; j++) {
			fp[j] = planes[(size_t)j * N + pixp], gp[j] = planes[(size_t)(kDenoiseFeat + j) * N + pixp];
			if constexpr (SLOPE) den[j] = feature_den(fp[j], gp[j], j, kf2, tau, mplanes[(size_t)j * N + pixp]);
			else den[j] = feature_den(fp[j], gp[j], j, kf2, tau);
		}
		p_fok = p_ok && fp[0] == fp[0];
	}

	for (int dy = -r; dy <= r; dy++) {
		for (int dx = -r; dx <= r; dx++) {
			const int db = dy * AW + dx;
#pragma unroll
			for (int s = 0; s < kSlots; s++) {
				const int j = tid + NT * s;
				if (j < PP) {
					const int ib = ia[s] + db;
					const double ub0 = U[ib];
					double t = 0.0;
					uint32_t taken = 0u;
					if (oka[s] && ub0 == ub0) {
						t = denoise_term(ua[s][0], ub0, va[s][0], V[ib], k2, alpha);
						t = t + denoise_term(ua[s][1], U[AA + ib], va[s][1], V[AA + ib], k2, alpha);
						t = t + denoise_term(ua[s][2], U[2 * AA + ib], va[s][2], V[2 * AA + ib], k2, alpha);
						taken = 1u;
					}
					T[j] = t, Tc[j] = taken;
				}
			}
			__syncthreads();
			for (int j = tid; j < (TH + 2 * f) * TW; j += NT) {
				const int ty = j / TW, x = j - ty * TW;
				const double *row = T + ty * PW + x;
				const uint32_t *crow = Tc + ty * PW + x;
				double h = row[0];
				uint32_t hc = crow[0];
				for (int o = 1; o <= 2 * f; o++) h = h + row[o], hc += crow[o];
				Hs[j] = h, Hc[j] = hc;
			}
			__syncthreads();
			if (p_ok && dx >= dx_lo && dx <= dx_hi && dy >= dy_lo && dy <= dy_hi) {
				const int iq = ip + db;
				const double uq0 = U[iq];
				if (uq0 == uq0) {
					double ds = Hs[py * TW + px];
					uint32_t cnt = Hc[py * TW + px];
					for (int o = 1; o <= 2 * f; o++) ds = ds + Hs[(py + o) * TW + px], cnt += Hc[(py + o) * TW + px];
					const double D = ds / (3.0 * (double)cnt);
					double w = exp(-(D > 0.0 ? D : 0.0));
					if constexpr (GUIDED) {
						if (p_fok) {
							const size_t pixq = (size_t)((int64_t)pixp + (int64_t)dy * (int64_t)W + dx); // (inside the frame: dx, dy are within the lo / hi bounds)
							const double fq0 = planes[pixq];
							if (fq0 == fq0) { // q is feature-valid too
								double Df = 0.0;
#pragma unroll
								for (int j = 0; j < kDenoiseFeat; j++) {
									const double fq = j == 0 ? fq0 : planes[(size_t)j * N + pixq], gq = planes[(size_t)(kDenoiseFeat + j) * N + pixq];
									const double phi = feature_phi(fp[j], gp[j], den[j], fq, gq);
									if (phi > Df) Df = phi; // (a NaN is skipped by the comparison)
								}
								const double wf = exp(-Df);
								if (wf < w) w = wf;
							}
						}
					}
					acc0 = acc0 + w * uq0, acc1 = acc1 + w * U[AA + iq], acc2 = acc2 + w * U[2 * AA + iq];
					wsum = wsum + w;
				}
			}
		}
	}

	if (!inside) return;
	const size_t o = ((size_t)gx + (size_t)gy * W) * 3;
	if (p_ok) {
		out[o + 0] = acc0 / wsum, out[o + 1] = acc1 / wsum, out[o + 2] = acc2 / wsum;
	} else { // not valid: the mean exactly as IEEE gives it (NaN stays NaN, n = 0 divides by zero)
		const double nd = (double)n_img[(size_t)gx + (size_t)gy * W];
		out[o + 0] = S[o + 0] / nd, out[o + 1] = S[o + 1] / nd, out[o + 2] = S[o + 2] / nd;
	}
}

size_t denoise_lds_bytes(uint32_t tile_width, uint32_t radius, uint32_t patch_radius) {
	const size_t AA = (size_t)(tile_width + 2u * (radius + patch_radius)) * (kDenoiseTile + 2u * (radius + patch_radius));
	const size_t PP = (size_t)(tile_width + 2u * patch_radius) * (kDenoiseTile + 2u * patch_radius), HH = (size_t)(kDenoiseTile + 2u * patch_radius) * tile_width;
	return (6u * AA + PP + HH) * sizeof(double) + (PP + HH) * sizeof(uint32_t);
}
uint32_t denoise_tile_width(uint32_t radius, uint32_t patch_radius) { return denoise_lds_bytes(32u, radius, patch_radius) <= kLdsBudgetBytes ? 32u : 24u; }

hipError_t launch_denoise_planes(hipStream_t stream, const DenoiseInput &in, uint32_t *n_img, double *feat_planes) {
	const bool guided = in.feat != nullptr;
	if (guided && (in.feat_sq == nullptr || feat_planes == nullptr)) return hipErrorInvalidValue;
	const size_t N = (size_t)in.W * in.H;
	hipError_t e = hipMemsetAsync(n_img, 0, N * sizeof(uint32_t), stream);
	if (e != hipSuccess) return e;
	if (in.n_rects) { // a column of workgroups per rect, enough for the largest (a full-frame rect is one rect)
		hipLaunchKernelGGL(count_image_kernel, dim3(in.n_rects, in.count_image_columns), dim3(256), 0, stream, in.rects, in.counts_a, in.W, n_img);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	if (guided) {
		hipLaunchKernelGGL(feature_planes_kernel, dim3((uint32_t)((N + 255u) / 256u)), dim3(256), 0, stream, in.accum_a, in.accum_sq_a, in.feat, in.feat_sq, n_img, N, feat_planes);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	return hipSuccess;
}

hipError_t launch_denoise_guided(hipStream_t stream, const DenoiseInput &in, const DenoiseWeights &w, uint32_t radius, uint32_t patch_radius, uint32_t *n_img,
                                 double *feat_planes, double *slope_planes, double *out) {
	if (radius > kDenoiseMaxRadius || patch_radius > kDenoiseMaxPatch) return hipErrorInvalidValue;
	const bool guided = in.feat != nullptr, sloped = guided && w.slope > 0.0;
	if (sloped && slope_planes == nullptr) return hipErrorInvalidValue;
	const double *accum = in.accum_a, *accum_sq = in.accum_sq_a;
	const uint32_t W = in.W, H = in.H;
	hipError_t e = launch_denoise_planes(stream, in, n_img, feat_planes);
	if (e != hipSuccess) return e;
	const uint32_t tw = denoise_tile_width(radius, patch_radius);
	const size_t lds = denoise_lds_bytes(tw, radius, patch_radius);
	if (lds > kLdsBudgetBytes) return hipErrorInvalidConfiguration; // (never within the limits: 145,152 B at r = 12, f = 4)
	if (sloped && (e = launch_feature_slope(stream, feat_planes, W, H, w.slope, slope_planes)) != hipSuccess) return e;
	const void *fn = sloped ? (tw == 32u ? reinterpret_cast<const void *>(&denoise_kernel<32, DenoiseSlope>) : reinterpret_cast<const void *>(&denoise_kernel<24, DenoiseSlope>))
	                 : guided ? (tw == 32u ? reinterpret_cast<const void *>(&denoise_kernel<32, DenoiseGuide>) : reinterpret_cast<const void *>(&denoise_kernel<24, DenoiseGuide>))
	                          : (tw == 32u ? reinterpret_cast<const void *>(&denoise_kernel<32>) : reinterpret_cast<const void *>(&denoise_kernel<24>));
	if ((e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return e;
	const dim3 grid((W + tw - 1u) / tw, (H + kDenoiseTile - 1u) / kDenoiseTile);
	const int ri = (int)radius, fi = (int)patch_radius;
	const double k2 = w.k * w.k, kf2 = w.k_f * w.k_f;
	if (sloped) {
		DenoiseSlope gs;
		gs.planes = feat_planes, gs.kf2 = kf2, gs.tau = w.tau, gs.m = slope_planes;
		if (tw == 32u) hipLaunchKernelGGL((denoise_kernel<32, DenoiseSlope>), grid, dim3(32 * kDenoiseTile), lds, stream, accum, accum_sq, n_img, W, H, ri, fi, k2, w.alpha, out, gs);
		else hipLaunchKernelGGL((denoise_kernel<24, DenoiseSlope>), grid, dim3(24 * kDenoiseTile), lds, stream, accum, accum_sq, n_img, W, H, ri, fi, k2, w.alpha, out, gs);
	} else if (guided) {
		const DenoiseGuide gd{feat_planes, kf2, w.tau};
		if (tw == 32u) hipLaunchKernelGGL((denoise_kernel<32, DenoiseGuide>), grid, dim3(32 * kDenoiseTile), lds, stream, accum, accum_sq, n_img, W, H, ri, fi, k2, w.alpha, out, gd);
		else hipLaunchKernelGGL((denoise_kernel<24, DenoiseGuide>), grid, dim3(24 * kDenoiseTile), lds, stream, accum, accum_sq, n_img, W, H, ri, fi, k2, w.alpha, out, gd);
	} else {
		if (tw == 32u) hipLaunchKernelGGL(denoise_kernel<32>, grid, dim3(32 * kDenoiseTile), lds, stream, accum, accum_sq, n_img, W, H, ri, fi, k2, w.alpha, out);
		else hipLaunchKernelGGL(denoise_kernel<24>, grid, dim3(24 * kDenoiseTile), lds, stream, accum, accum_sq, n_img, W, H, ri, fi, k2, w.alpha, out);
	}
	return hipGetLastError();
}

} // namespace rmd
