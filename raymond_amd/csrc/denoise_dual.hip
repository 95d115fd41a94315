// Dual-buffer (cross) non-local means and its per-pixel error estimate (rmd_denoise_dual, rmd_tile_error_dual; include/raymond_hip.h states
// the definition, DESIGN.md section 13 the structure and its cost).  A translation unit of its own: the code objects of denoise.hip and of the
// render kernels do not change.
//
// dual_planes_kernel       — per pixel, both halves' u and v (denoise_device.hpp: dual_planes_pixel, denoise_kernel's staging arithmetic) into twelve planar images of W*H
//                            doubles: half h's u in planes 6h + c, its v in planes 6h + 3 + c.  A pixel that is not DUAL-VALID keeps a NaN in
//                            the u of channel 0 of BOTH halves, so one test reads "valid" as dual-valid everywhere.
// denoise_dual_kernel<TW>  — one cross pass: the weights from the six planes of the WEIGHT half, staged into LDS as denoise_kernel stages its
//                            own (same apron, term image, row and column sums, two barriers per offset, each window summed directly), applied
//                            to the u of the VALUE half.  Launched twice with the roles swapped: f_A (weights from B), then f_B (weights from A).
//                            REGION = false: workgroup (bx, by) owns the TW x 16 pixels at (bx * TW, by * 16), the whole frame.  REGION = true
//                            (rmd_denoise_dual_region): workgroup b owns the pixels of entry b of a BLOCK TABLE — a DualBlock: the block's origin
//                            and the far corner (exclusive) of the region rect it was cut from — and writes only the pixels before that corner.
//                            Nothing else differs: a pixel's value does not depend on where its workgroup's origin lies.
//   Why six planes in LDS and the value half from global memory, not nine planes under a narrower tile: at r = 10, f = 3 nine f64 planes of a
//   32-wide tile's apron are 175 KB, over the 160 KB budget, and a 24-wide tile's 151 KB leave no room for the term image (165 KB together).
//   Nine planes fit only from TW = 16 down (137 KB): four waves a workgroup, one workgroup a CU, 6.9 apron pixels staged and 1.9 term
//   positions computed per output pixel against 4.8 and 1.6 at TW = 32 — and at r = 12, f = 4 not even TW = 16 fits (166 KB).  The
//   value half is read once per taken neighbour, three doubles from planar images: neighbouring lanes read neighbouring doubles and
//   consecutive offsets shift by one pixel, the access the guided kernel makes fourteen times per neighbour and found to be cache hits.  The
//   LDS layout, its size (denoise_lds_bytes) and the tile width (denoise_tile_width) are therefore denoise_kernel's own.
// dual_combine_kernel      — out = (n_A f_A + n_B f_B) / (n_A + n_B) and err = mean_c ((f_A - f_B) / 2)^2 for a dual-valid pixel, the merged
//                            mean and NaN for any other.  dual_combine_region_kernel: the same per pixel, over a block table's pixels only.
// GUIDED (rmd_denoise_dual_guided; denoise_dual_kernel<TW, REGION, DualGuide>, instantiations of their own so that the unguided four are compiled
// exactly as without the feature): dual_feature_planes_kernel writes the planar per-pixel f and g of the feature buffers at their OWN count n_F
// (14 planes of W*H doubles; a pixel that is not feature-valid — dual-valid by dual_planes_kernel's mark, n_F >= 2, fourteen finite sums — keeps a
// NaN in its f of channel 0), and step 3 of each cross pass makes rmd_denoise_guided's w_f of the pixel pair and takes min(w, w_f): p's seven f, g
// and denominators in registers, q's fourteen values per taken neighbour from the planes in global memory.  w_f is evaluated in BOTH passes
// (DESIGN.md section 15); the LDS layout is unchanged.
// SLOPE (the dual _slope calls at slope > 0): one more optional argument after the DualGuide, a DualSlope — the seven planes m that
// denoise.hip's feature_slope_kernel makes of the f planes, over the whole frame in the region form too; the pass reads p's seven m once, where the
// denominators are made.  Instantiations of their own once more: the twelve without it keep their arguments and their instructions.
// SELECTION (rmd_denoise_dual_select): the whole-frame cross pass takes one more optional trailing argument, a DualGain, and then
// also writes g(p) = w(p, p) / sum_q w(p, q), the derivative of f(p) by the value half's own u(p) — instantiations of their own again, so the eight
// above keep their arguments and their instructions.  dual_sure_kernel makes a candidate's per-pixel SURE from the planes, its two f and the two g
// images; dual_winner_kernel the windowed means of every candidate's SURE (dual_window_mean) and the index of the smallest; dual_blend_kernel the
// weights m_i from the winners around the pixel, the blended f_A and f_B, and then dual_combine_pixel itself.
// tile_error_dual_kernel   — one workgroup per rect: sqrt(sum err / pixels), +inf when an err of the rect is NaN.
// f64 throughout, built with -ffp-contract=off like the rest of the library.
#include <hip/hip_runtime.h>

#include "denoise_device.hpp"

namespace rmd {

// (count_image_kernel of denoise.hip, for two count arrays at once: n_a and n_b are zeroed by the caller)
__global__ __launch_bounds__(256) void dual_count_image_kernel(const rmd_tile_rect *__restrict__ rects, const uint32_t *__restrict__ counts_a,
                                                               const uint32_t *__restrict__ counts_b, uint32_t W, uint32_t *__restrict__ n_a,
                                                               uint32_t *__restrict__ n_b) {
	const rmd_tile_rect r = rects[blockIdx.x];
	const uint32_t na = counts_a[blockIdx.x], nb = counts_b[blockIdx.x];
	const uint64_t n_px = (uint64_t)r.width * r.height;
	for (uint64_t i = (uint64_t)blockIdx.y * 256u + threadIdx.x; i < n_px; i += (uint64_t)gridDim.y * 256u) {
		const size_t p = rect_pixel(r, i, W);
		n_a[p] = na, n_b[p] = nb;
	}
}

__global__ __launch_bounds__(256) void dual_planes_kernel(const double *__restrict__ SA, const double *__restrict__ QA, const double *__restrict__ SB,
                                                          const double *__restrict__ QB, const uint32_t *__restrict__ n_a, const uint32_t *__restrict__ n_b,
                                                          size_t N, double *__restrict__ planes) {
	const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i < N) dual_planes_pixel(SA, QA, SB, QB, n_a[i], n_b[i], i, N, planes);
}

// (count_image_kernel of denoise.hip for the features' own counts: n_f is zeroed by the caller)
__global__ __launch_bounds__(256) void dual_feature_count_image_kernel(const rmd_tile_rect *__restrict__ rects, const uint32_t *__restrict__ counts_f, uint32_t W,
                                                                       uint32_t *__restrict__ n_f) {
	const rmd_tile_rect r = rects[blockIdx.x];
	const uint32_t nf = counts_f[blockIdx.x];
	const uint64_t n_px = (uint64_t)r.width * r.height;
	for (uint64_t i = (uint64_t)blockIdx.y * 256u + threadIdx.x; i < n_px; i += (uint64_t)gridDim.y * 256u) n_f[rect_pixel(r, i, W)] = nf;
}

// feature_planes_pixel at the features' own count n_F, seeded with the dual-validity: planes[i], dual_planes_kernel's mark, is no NaN
__global__ __launch_bounds__(256) void dual_feature_planes_kernel(const double *__restrict__ planes, const double *__restrict__ F, const double *__restrict__ G,
                                                                  const uint32_t *__restrict__ n_f, size_t N, double *__restrict__ fplanes) {
	const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= N) return;
	const double ua0 = planes[i];
	feature_planes_pixel(F, G, i, n_f[i], ua0 == ua0, N, fplanes);
}

// the guided kernel's extra arguments: the planar f and g images, k_f^2 and tau (denoise.hip's DenoiseGuide; a type of its own, which the kernels' names carry)
struct DualGuide {
	const double *planes;
	double kf2, tau;
};
// the _slope calls' extra argument at slope > 0 (after the DualGuide): feature_slope_kernel's seven planes m (denoise.hip)
struct DualSlope {
	const double *m;
};
// the selecting call's extra argument: the W*H image that receives g(p) = w(p, p) / sum_q w(p, q) at the pixels where fout is written
struct DualGain {
	double *g;
};
// the argument of type T among a kernel's trailing pack
template <class T, class A, class... R>
__device__ inline T dual_pick(A a, R... rest) {
	if constexpr (__is_same(T, A)) return a;
	else return dual_pick<T>(rest...);
}

// Pw: the weight half's six planes (u, then v); Uv: the value half's three u planes; fout: W*H*3 doubles, pixel-interleaved, written at dual-valid
// pixels only (dual_combine_kernel gives the others their value).
// table: REGION only (null otherwise), one entry per workgroup.
// GUIDED is the presence of a DualGuide argument: denoise_dual_kernel<TW, REGION> (no such argument) keeps the signature and the code it had before the
// feature weight existed, denoise_dual_kernel<TW, REGION, DualGuide> is the guided instantiation.  GAIN is the presence of a DualGain argument (after the
// DualGuide, if there is one): the weight the loop makes at offset (0, 0) is kept, and g = that weight / wsum is written beside fout.
template <int TW, bool REGION, class... G>
__global__ __launch_bounds__(TW * 16) void denoise_dual_kernel(const double *__restrict__ Pw, const double *__restrict__ Uv, const DualBlock *__restrict__ table, uint32_t W,
                                                               uint32_t H, int r, int f, double k2, double alpha, double *__restrict__ fout, G... guide) {
	constexpr bool GUIDED = (__is_same(G, DualGuide) || ...), GAIN = (__is_same(G, DualGain) || ...), SLOPE = (__is_same(G, DualSlope) || ...);
	static_assert(sizeof...(G) == (GUIDED ? 1 : 0) + (SLOPE ? 1 : 0) + (GAIN ? 1 : 0) && (GUIDED || !SLOPE), "at most one DualGuide, with it at most one DualSlope, then at most one DualGain");
	[[maybe_unused]] const double *fplanes = nullptr;
	[[maybe_unused]] double kf2 = 0.0, tau = 0.0;
	if constexpr (GUIDED) {
		const DualGuide gd = dual_pick<DualGuide>(guide...);
		fplanes = gd.planes, kf2 = gd.kf2, tau = gd.tau;
	}
	[[maybe_unused]] const double *mplanes = nullptr; // SLOPE: p's seven m are read once, where den is made; the per-pair loop is the guided one's
	if constexpr (SLOPE) mplanes = dual_pick<DualSlope>(guide...).m;
	[[maybe_unused]] double *gout = nullptr;
	[[maybe_unused]] double wcentre = 0.0; // GAIN: w(p, p) — set for every p_ok pixel, whose own offset (0, 0) is always taken
	if constexpr (GAIN) gout = dual_pick<DualGain>(guide...).g;
	extern __shared__ double lds[];
	constexpr int TH = (int)kDenoiseTile, NT = TW * TH;
	const int R = r + f, AW = TW + 2 * R, AA = AW * (TH + 2 * R), PW = TW + 2 * f, PP = PW * (TH + 2 * f);
	double *U = lds, *V = lds + 3 * AA;           // planes c * AA + (apron row * AW + apron column)
	double *T = lds + 6 * AA, *Hs = T + PP;        // the term image (TH + 2f rows of PW) and its row sums (TH + 2f rows of TW)
	uint32_t *Tc = reinterpret_cast<uint32_t *>(Hs + (TH + 2 * f) * TW), *Hc = Tc + PP;
	int64_t x0, y0, x_end, y_end; // the tile's origin; the pixels it may write lie before (x_end, y_end)
	if constexpr (REGION) {
		const DualBlock e = table[blockIdx.x];
		x0 = e.x0, y0 = e.y0, x_end = e.x_end, y_end = e.y_end;
	} else {
		x0 = (int64_t)blockIdx.x * TW, y0 = (int64_t)blockIdx.y * TH, x_end = W, y_end = H;
	}
	const int tid = threadIdx.x;
	const size_t N = (size_t)W * H;

	for (int i = tid; i < AA; i += NT) {
		const int ly = i / AW, lx = i - ly * AW;
		const int64_t gx = min(max(x0 - R + lx, (int64_t)0), (int64_t)W - 1), gy = min(max(y0 - R + ly, (int64_t)0), (int64_t)H - 1);
		const size_t pix = (size_t)gx + (size_t)gy * W;
#pragma unroll
		for (int c = 0; c < 3; c++) U[c * AA + i] = Pw[(size_t)c * N + pix], V[c * AA + i] = Pw[(size_t)(3 + c) * N + pix];
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
	const bool inside = gx < x_end && gy < y_end; // (a table entry's far corner lies inside the frame)
	const int ip = (py + R) * AW + (px + R);
	const bool p_ok = inside && U[ip] == U[ip];
	const int dx_lo = (int)max((int64_t)-r, -gx), dx_hi = (int)min((int64_t)r, (int64_t)W - 1 - gx);
	const int dy_lo = (int)max((int64_t)-r, -gy), dy_hi = (int)min((int64_t)r, (int64_t)H - 1 - gy);
	const size_t pixp = inside ? (size_t)gx + (size_t)gy * W : 0;
	double acc0 = -0.0, acc1 = -0.0, acc2 = -0.0, wsum = -0.0; // -0.0 + x == x for every x, so r = 0 gives the value half's u bit for bit
	// GUIDED: this pixel's features, their variances and the denominators of Phi_j(p, .)
	[[maybe_unused]] double fp[kDenoiseFeat], gp[kDenoiseFeat], den[kDenoiseFeat];
	[[maybe_unused]] bool p_fok = false;
	if constexpr (GUIDED) {
#pragma unroll
		for (int j = 0; j < kDenoiseFeat; j++) {
			fp[j] = fplanes[(size_t)j * N + pixp], gp[j] = fplanes[(size_t)(kDenoiseFeat + j) * N + pixp];
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
				const double wq0 = U[ip + db];
				if (wq0 == wq0) { // q is dual-valid
					double ds = Hs[py * TW + px];
					uint32_t cnt = Hc[py * TW + px];
					for (int o = 1; o <= 2 * f; o++) ds = ds + Hs[(py + o) * TW + px], cnt += Hc[(py + o) * TW + px];
					const double D = ds / (3.0 * (double)cnt);
					double w = exp(-(D > 0.0 ? D : 0.0));
					const size_t pixq = (size_t)((int64_t)pixp + (int64_t)dy * (int64_t)W + dx); // (inside the frame: dx, dy are within the lo / hi bounds)
					if constexpr (GUIDED) {
						if (p_fok) {
							const double fq0 = fplanes[pixq];
							if (fq0 == fq0) { // q is feature-valid too
								double Df = 0.0;
#pragma unroll
								for (int j = 0; j < kDenoiseFeat; j++) {
									const double fq = j == 0 ? fq0 : fplanes[(size_t)j * N + pixq], gq = fplanes[(size_t)(kDenoiseFeat + j) * N + pixq];
									const double phi = feature_phi(fp[j], gp[j], den[j], fq, gq);
									if (phi > Df) Df = phi; // (a NaN is skipped by the comparison)
								}
								const double wf = exp(-Df);
								if (wf < w) w = wf;
							}
						}
					}
					acc0 = acc0 + w * Uv[pixq], acc1 = acc1 + w * Uv[N + pixq], acc2 = acc2 + w * Uv[2 * N + pixq];
					wsum = wsum + w;
					if constexpr (GAIN) {
						if (dx == 0 && dy == 0) wcentre = w;
					}
				}
			}
		}
	}

	if (p_ok) {
		const size_t o = pixp * 3;
		fout[o + 0] = acc0 / wsum, fout[o + 1] = acc1 / wsum, fout[o + 2] = acc2 / wsum;
		if constexpr (GAIN) gout[pixp] = wcentre / wsum;
	}
}

// fa = out (read before it is written, in place), fb: the two cross passes' results.  Dual-valid p: dual_combine of them; any other p: dual_merged.  err may be null.
__device__ inline void dual_combine_pixel(const double *__restrict__ SA, const double *__restrict__ SB, const uint32_t *__restrict__ n_a,
                                          const uint32_t *__restrict__ n_b, const double *__restrict__ planes, const double *__restrict__ fb, size_t i, double *out,
                                          double *__restrict__ err) {
	const double na = (double)n_a[i], nb = (double)n_b[i];
	const double ua0 = planes[i];
	if (ua0 == ua0) {
		const double a[3] = {out[i * 3 + 0], out[i * 3 + 1], out[i * 3 + 2]}, b[3] = {fb[i * 3 + 0], fb[i * 3 + 1], fb[i * 3 + 2]};
		dual_combine(a, b, na, nb, i, out, err);
	} else {
		dual_merged(SA, SB, na, nb, i, out, err);
	}
}
__global__ __launch_bounds__(256) void dual_combine_kernel(const double *__restrict__ SA, const double *__restrict__ SB, const uint32_t *__restrict__ n_a,
                                                           const uint32_t *__restrict__ n_b, const double *__restrict__ planes, const double *__restrict__ fb,
                                                           size_t N, double *out, double *__restrict__ err) {
	const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i < N) dual_combine_pixel(SA, SB, n_a, n_b, planes, fb, i, out, err);
}
// One workgroup of tw * 16 threads per block-table entry, thread t at (t % tw, t / tw) from the entry's origin: the pixels denoise_dual_kernel wrote.
__global__ __launch_bounds__(512) void dual_combine_region_kernel(const double *__restrict__ SA, const double *__restrict__ SB, const uint32_t *__restrict__ n_a,
                                                                  const uint32_t *__restrict__ n_b, const double *__restrict__ planes, const double *__restrict__ fb,
                                                                  const DualBlock *__restrict__ table, uint32_t tw, uint32_t W, double *out, double *__restrict__ err) {
	const DualBlock e = table[blockIdx.x];
	const uint32_t x = e.x0 + threadIdx.x % tw, y = e.y0 + threadIdx.x / tw; // (no wrap: the origin lies before the far corner, 512 pixels at most beyond it)
	if (x < e.x_end && y < e.y_end) dual_combine_pixel(SA, SB, n_a, n_b, planes, fb, (size_t)x + (size_t)y * W, out, err);
}

template <int TW, bool REGION>
static hipError_t launch_dual_pass(hipStream_t stream, dim3 grid, size_t lds, const double *Pw, const double *Uv, const DualBlock *table, uint32_t W, uint32_t H, int r,
                                   int f, double k2, double alpha, double *fout, const DualGuide *gd, const DualSlope *gs) {
	if (gd && gs) hipLaunchKernelGGL((denoise_dual_kernel<TW, REGION, DualGuide, DualSlope>), grid, dim3(TW * kDenoiseTile), lds, stream, Pw, Uv, table, W, H, r, f, k2, alpha, fout, *gd, *gs);
	else if (gd) hipLaunchKernelGGL((denoise_dual_kernel<TW, REGION, DualGuide>), grid, dim3(TW * kDenoiseTile), lds, stream, Pw, Uv, table, W, H, r, f, k2, alpha, fout, *gd);
	else hipLaunchKernelGGL((denoise_dual_kernel<TW, REGION>), grid, dim3(TW * kDenoiseTile), lds, stream, Pw, Uv, table, W, H, r, f, k2, alpha, fout);
	return hipGetLastError();
}
template <int TW, bool REGION>
static const void *dual_pass_fn(bool guided, bool sloped) {
	return sloped ? reinterpret_cast<const void *>(&denoise_dual_kernel<TW, REGION, DualGuide, DualSlope>)
	     : guided ? reinterpret_cast<const void *>(&denoise_dual_kernel<TW, REGION, DualGuide>) : reinterpret_cast<const void *>(&denoise_dual_kernel<TW, REGION>);
}

// What every dual call makes first, once — also the filters of other units (denoise_atrous_dual.hip): both halves' count images and the twelve planes;
// with features also their count image and their fourteen planes (which read the dual-validity mark dual_planes_kernel has just left)
hipError_t launch_dual_planes(hipStream_t stream, const DenoiseInput &in, uint32_t *n_img, double *planes, uint32_t *n_f_img, double *feat_planes) {
	const size_t N = (size_t)in.W * in.H;
	uint32_t *n_a = n_img, *n_b = n_img + N;
	hipError_t e = hipMemsetAsync(n_img, 0, 2u * N * sizeof(uint32_t), stream);
	if (e != hipSuccess) return e;
	if (in.n_rects) {
		hipLaunchKernelGGL(dual_count_image_kernel, dim3(in.n_rects, in.count_image_columns), dim3(256), 0, stream, in.rects, in.counts_a, in.counts_b, in.W, n_a, n_b);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	const uint32_t blocks = (uint32_t)((N + 255u) / 256u);
	hipLaunchKernelGGL(dual_planes_kernel, dim3(blocks), dim3(256), 0, stream, in.accum_a, in.accum_sq_a, in.accum_b, in.accum_sq_b, n_a, n_b, N, planes);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (in.feat) {
		if ((e = hipMemsetAsync(n_f_img, 0, N * sizeof(uint32_t), stream)) != hipSuccess) return e;
		if (in.n_rects) {
			hipLaunchKernelGGL(dual_feature_count_image_kernel, dim3(in.n_rects, in.count_image_columns), dim3(256), 0, stream, in.rects, in.counts_f, in.W, n_f_img);
			if ((e = hipGetLastError()) != hipSuccess) return e;
		}
		hipLaunchKernelGGL(dual_feature_planes_kernel, dim3(blocks), dim3(256), 0, stream, planes, in.feat, in.feat_sq, n_f_img, N, feat_planes);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	return hipSuccess;
}

hipError_t launch_denoise_dual(hipStream_t stream, const DenoiseInput &in, const DenoiseWeights &w, uint32_t radius, uint32_t patch_radius, uint32_t *n_img, double *planes,
                               double *f_b, uint32_t *n_f_img, double *feat_planes, double *slope_planes, const DualBlock *table, uint32_t n_blocks, double *out,
                               double *err) {
	if (radius > kDenoiseMaxRadius || patch_radius > kDenoiseMaxPatch) return hipErrorInvalidValue;
	const bool guided = in.feat != nullptr, sloped = guided && w.slope > 0.0;
	if (guided && (in.feat_sq == nullptr || n_f_img == nullptr || feat_planes == nullptr || (in.n_rects && in.counts_f == nullptr))) return hipErrorInvalidValue;
	if (sloped && slope_planes == nullptr) return hipErrorInvalidValue;
	if (table && n_blocks == 0) return hipSuccess; // a region without pixels: nothing would read the planes
	const double *accum_a = in.accum_a, *accum_b = in.accum_b;
	const uint32_t W = in.W, H = in.H;
	const size_t N = (size_t)W * H;
	uint32_t *n_a = n_img, *n_b = n_img + N;
	hipError_t e = launch_dual_planes(stream, in, n_img, planes, n_f_img, feat_planes);
	if (e != hipSuccess) return e;
	const uint32_t blocks = (uint32_t)((N + 255u) / 256u);
	const uint32_t tw = denoise_tile_width(radius, patch_radius);
	const size_t lds = denoise_lds_bytes(tw, radius, patch_radius);
	if (lds > kLdsBudgetBytes) return hipErrorInvalidConfiguration; // (never within the limits, as for denoise_kernel)
	if (sloped && (e = launch_feature_slope(stream, feat_planes, W, H, w.slope, slope_planes)) != hipSuccess) return e; // (whole-frame in the region form too, as the planes are)
	const void *fn = table ? (tw == 32u ? dual_pass_fn<32, true>(guided, sloped) : dual_pass_fn<24, true>(guided, sloped))
	                       : (tw == 32u ? dual_pass_fn<32, false>(guided, sloped) : dual_pass_fn<24, false>(guided, sloped));
	if ((e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return e;
	const dim3 grid = table ? dim3(n_blocks) : dim3((W + tw - 1u) / tw, (H + kDenoiseTile - 1u) / kDenoiseTile);
	const int ri = (int)radius, fi = (int)patch_radius;
	const double k2 = w.k * w.k, alpha = w.alpha;
	const DualGuide gd{feat_planes, w.k_f * w.k_f, w.tau};
	const DualGuide *gp = guided ? &gd : nullptr;
	const DualSlope gs{slope_planes};
	const DualSlope *sp = sloped ? &gs : nullptr;
	const double *PA = planes, *PB = planes + 6u * N;
	for (int pass = 0; pass < 2; pass++) { // f_A: weights from B applied to u_A, into out; f_B: weights from A applied to u_B, into f_b (guided: the same w_f in both)
		const double *Pw = pass == 0 ? PB : PA, *Uv = pass == 0 ? PA : PB;
		double *fout = pass == 0 ? out : f_b;
		if (table && tw == 32u) e = launch_dual_pass<32, true>(stream, grid, lds, Pw, Uv, table, W, H, ri, fi, k2, alpha, fout, gp, sp);
		else if (table) e = launch_dual_pass<24, true>(stream, grid, lds, Pw, Uv, table, W, H, ri, fi, k2, alpha, fout, gp, sp);
		else if (tw == 32u) e = launch_dual_pass<32, false>(stream, grid, lds, Pw, Uv, table, W, H, ri, fi, k2, alpha, fout, gp, sp);
		else e = launch_dual_pass<24, false>(stream, grid, lds, Pw, Uv, table, W, H, ri, fi, k2, alpha, fout, gp, sp);
		if (e != hipSuccess) return e;
	}
	if (table) hipLaunchKernelGGL(dual_combine_region_kernel, grid, dim3(tw * kDenoiseTile), 0, stream, accum_a, accum_b, n_a, n_b, planes, f_b, table, tw, W, out, err);
	else hipLaunchKernelGGL(dual_combine_kernel, dim3(blocks), dim3(256), 0, stream, accum_a, accum_b, n_a, n_b, planes, f_b, N, out, err);
	return hipGetLastError();
}

// ---------------------------------------------------------------- rmd_denoise_dual_select
// One candidate's per-pixel SURE.  Half X with u, v its planes, f its cross pass's result and g its gain image: t_c = ((d*d) - v_c) + ((2*v_c) * g) with
// d = f_c - u_c; sure_X = ((t_0 + t_1) + t_2) / 3.  sure = ((n_A * sure_A) + (n_B * sure_B)) / (n_A + n_B); NaN at a pixel that is not dual-valid.
__global__ __launch_bounds__(256) void dual_sure_kernel(const double *__restrict__ planes, const double *__restrict__ fa, const double *__restrict__ fb,
                                                        const double *__restrict__ ga, const double *__restrict__ gb, const uint32_t *__restrict__ n_a,
                                                        const uint32_t *__restrict__ n_b, size_t N, double *__restrict__ sure) {
	const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= N) return;
	const double ua0 = planes[i];
	if (!(ua0 == ua0)) {
		sure[i] = __builtin_nan("");
		return;
	}
	double sx[2];
#pragma unroll
	for (int h = 0; h < 2; h++) {
		const double *f = h ? fb : fa;
		const double g = h ? gb[i] : ga[i];
		double t = 0.0;
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const double u = planes[(size_t)(6 * h + c) * N + i], v = planes[(size_t)(6 * h + 3 + c) * N + i];
			const double d = f[i * 3 + c] - u;
			const double tc = (d * d - v) + (2.0 * v) * g;
			t = c == 0 ? tc : t + tc;
		}
		sx[h] = t / 3.0;
	}
	const double na = (double)n_a[i], nb = (double)n_b[i];
	sure[i] = (na * sx[0] + nb * sx[1]) / (na + nb);
}

// The mean of `img` over the dual-valid pixels (planes[q] is no NaN) of the (2*win + 1)^2 window around (x, y) that lie inside the frame: 0.0, then every such
// pixel's value added in raster order, divided by their number (0 / 0 = NaN where there is none).
__device__ inline double dual_window_mean(const double *__restrict__ img, const double *__restrict__ planes, int64_t x, int64_t y, int64_t W, int64_t H, int win) {
	double s = 0.0;
	uint32_t cnt = 0u;
	for (int64_t qy = y - win; qy <= y + win; qy++) {
		if (qy < 0 || qy >= H) continue;
		for (int64_t qx = x - win; qx <= x + win; qx++) {
			if (qx < 0 || qx >= W) continue;
			const size_t q = (size_t)qx + (size_t)qy * (size_t)W;
			const double m = planes[q];
			if (m == m) s = s + img[q], cnt++;
		}
	}
	return s / (double)cnt;
}

// win[p] = the lowest index i with the smallest E_i(p), the window mean of candidate i's SURE (image i of `sure`, N doubles apart at stride `stride`);
// a NaN E loses to any number; all NaN: 0.  0xFFFFFFFF at a pixel that is not dual-valid.
__global__ __launch_bounds__(256) void dual_winner_kernel(const double *__restrict__ sure, size_t stride, uint32_t n_cands, const double *__restrict__ planes, uint32_t W,
                                                          uint32_t H, int win_radius, uint32_t *__restrict__ win) {
	const size_t N = (size_t)W * H, i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= N) return;
	const double ua0 = planes[i];
	if (!(ua0 == ua0)) {
		win[i] = 0xFFFFFFFFu;
		return;
	}
	const int64_t x = (int64_t)(i % W), y = (int64_t)(i / W);
	uint32_t best = 0u;
	double eb = dual_window_mean(sure, planes, x, y, W, H, win_radius);
	for (uint32_t c = 1; c < n_cands; c++) {
		const double e = dual_window_mean(sure + (size_t)c * stride, planes, x, y, W, H, win_radius);
		if (e < eb || (eb != eb && e == e)) best = c, eb = e;
	}
	win[i] = best;
}

// Per pixel p.  Dual-valid: cnt_i = the dual-valid in-frame pixels q of the (2*sel + 1)^2 window with win[q] = i, total = all of them (p is one), m_i =
// cnt_i / total; f_X = m_0 * f_X,0, then + m_i * f_X,i in index order, per channel; f_A goes to out and f_B to candidate 0's f_B image (only p's own
// entries of either are read here, by this thread), and dual_combine_pixel makes out and err of them.  sure_out = the same sum over the SURE images.
// Any other pixel: dual_combine_pixel's merged mean and NaN, sure_out NaN.  cand: candidate i's images at cand + i * stride — f_A (3N), f_B (3N), SURE (N).
__global__ __launch_bounds__(256) void dual_blend_kernel(const double *__restrict__ SA, const double *__restrict__ SB, const uint32_t *__restrict__ n_a,
                                                         const uint32_t *__restrict__ n_b, const double *__restrict__ planes, double *cand, size_t stride,
                                                         uint32_t n_cands, const uint32_t *__restrict__ win, uint32_t W, uint32_t H, int sel_radius, double *out,
                                                         double *__restrict__ err, double *__restrict__ sure_out, uint32_t *__restrict__ win_out) {
	const size_t N = (size_t)W * H, i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= N) return;
	const double ua0 = planes[i];
	if (ua0 == ua0) {
		const int64_t x = (int64_t)(i % W), y = (int64_t)(i / W);
		uint32_t cnt[kDenoiseMaxCandidates] = {0u, 0u, 0u, 0u}, total = 0u;
		for (int64_t qy = y - sel_radius; qy <= y + sel_radius; qy++) {
			if (qy < 0 || qy >= (int64_t)H) continue;
			for (int64_t qx = x - sel_radius; qx <= x + sel_radius; qx++) {
				if (qx < 0 || qx >= (int64_t)W) continue;
				const uint32_t w = win[(size_t)qx + (size_t)qy * W];
				if (w != 0xFFFFFFFFu) {
					total++;
#pragma unroll
					for (uint32_t c = 0; c < kDenoiseMaxCandidates; c++) cnt[c] += w == c ? 1u : 0u;
				}
			}
		}
		double fa[3], fb[3], su = 0.0;
#pragma unroll
		for (uint32_t c = 0; c < kDenoiseMaxCandidates; c++) {
			if (c < n_cands) {
				const double m = (double)cnt[c] / (double)total;
				const double *ca = cand + (size_t)c * stride, *cb = ca + 3u * N, *cs = ca + 6u * N;
#pragma unroll
				for (int ch = 0; ch < 3; ch++) {
					const double pa = m * ca[i * 3 + ch], pb = m * cb[i * 3 + ch];
					fa[ch] = c == 0 ? pa : fa[ch] + pa, fb[ch] = c == 0 ? pb : fb[ch] + pb;
				}
				const double ps = m * cs[i];
				su = c == 0 ? ps : su + ps;
			}
		}
#pragma unroll
		for (int ch = 0; ch < 3; ch++) out[i * 3 + ch] = fa[ch], cand[3u * N + i * 3 + ch] = fb[ch];
		if (sure_out) sure_out[i] = su;
	} else if (sure_out) sure_out[i] = __builtin_nan("");
	if (win_out) win_out[i] = win[i];
	dual_combine_pixel(SA, SB, n_a, n_b, planes, cand + 3u * N, i, out, err);
}

// a whole-frame cross pass that also writes its gain image
template <int TW>
static hipError_t launch_dual_pass_gain(hipStream_t stream, dim3 grid, size_t lds, const double *Pw, const double *Uv, uint32_t W, uint32_t H, int r, int f, double k2,
                                        double alpha, double *fout, const DualGuide *gd, const DualSlope *gs, DualGain gn) {
	const DualBlock *none = nullptr;
	if (gd && gs) {
		hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&denoise_dual_kernel<TW, false, DualGuide, DualSlope, DualGain>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e;
		hipLaunchKernelGGL((denoise_dual_kernel<TW, false, DualGuide, DualSlope, DualGain>), grid, dim3(TW * kDenoiseTile), lds, stream, Pw, Uv, none, W, H, r, f, k2, alpha, fout, *gd, *gs, gn);
	} else if (gd) {
		hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&denoise_dual_kernel<TW, false, DualGuide, DualGain>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e;
		hipLaunchKernelGGL((denoise_dual_kernel<TW, false, DualGuide, DualGain>), grid, dim3(TW * kDenoiseTile), lds, stream, Pw, Uv, none, W, H, r, f, k2, alpha, fout, *gd, gn);
	} else {
		hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&denoise_dual_kernel<TW, false, DualGain>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e;
		hipLaunchKernelGGL((denoise_dual_kernel<TW, false, DualGain>), grid, dim3(TW * kDenoiseTile), lds, stream, Pw, Uv, none, W, H, r, f, k2, alpha, fout, gn);
	}
	return hipGetLastError();
}

hipError_t launch_denoise_dual_select(hipStream_t stream, const DenoiseInput &in, uint32_t radius, uint32_t patch_radius, const rmd_denoise_candidate *cands,
                                      const double *cand_slopes, uint32_t n_cands, uint32_t sure_window, uint32_t select_window, uint32_t *n_img, double *planes,
                                      double *cand_img, double *gain, uint32_t *win_img, uint32_t *n_f_img, double *feat_planes, double *slope_planes, double *out,
                                      double *err, double *sure, uint32_t *win) {
	if (radius > kDenoiseMaxRadius || patch_radius > kDenoiseMaxPatch || n_cands == 0 || n_cands > kDenoiseMaxCandidates || sure_window > kDenoiseMaxSelectWindow ||
	    select_window > kDenoiseMaxSelectWindow)
		return hipErrorInvalidValue;
	bool any_guided = false;
	for (uint32_t i = 0; i < n_cands; i++) any_guided = any_guided || cands[i].guided != 0u;
	if (any_guided && (in.feat == nullptr || in.feat_sq == nullptr || n_f_img == nullptr || feat_planes == nullptr || (in.n_rects && in.counts_f == nullptr)))
		return hipErrorInvalidValue;
	const double *accum_a = in.accum_a, *accum_b = in.accum_b;
	const uint32_t W = in.W, H = in.H;
	const size_t N = (size_t)W * H;
	uint32_t *n_a = n_img, *n_b = n_img + N;
	// once per call, whatever the number of candidates: k_f and tau enter the feature weight through denominators the kernel makes itself
	DenoiseInput pre = in;
	if (!any_guided) pre.feat = nullptr;
	hipError_t e = launch_dual_planes(stream, pre, n_img, planes, n_f_img, feat_planes);
	if (e != hipSuccess) return e;
	const uint32_t blocks = (uint32_t)((N + 255u) / 256u);
	const uint32_t tw = denoise_tile_width(radius, patch_radius);
	const size_t lds = denoise_lds_bytes(tw, radius, patch_radius);
	if (lds > kLdsBudgetBytes) return hipErrorInvalidConfiguration;
	const dim3 grid((W + tw - 1u) / tw, (H + kDenoiseTile - 1u) / kDenoiseTile);
	const int ri = (int)radius, fi = (int)patch_radius;
	const double *PA = planes, *PB = planes + 6u * N;
	const size_t stride = 7u * N; // a candidate's images: f_A (3N), f_B (3N), SURE (N)
	double *g_a = gain, *g_b = gain + N;
	double made_slope = 0.0; // the slope the one set of slope planes holds (0: none yet): remade when a guided candidate's differs
	for (uint32_t i = 0; i < n_cands; i++) {
		const rmd_denoise_candidate &c = cands[i];
		const double k2 = c.k * c.k;
		const DualGuide gd{feat_planes, c.k_f * c.k_f, c.tau};
		const DualGuide *gp = c.guided ? &gd : nullptr;
		const double slope = c.guided && cand_slopes ? cand_slopes[i] : 0.0;
		const DualSlope gs{slope_planes};
		const DualSlope *sp = slope > 0.0 ? &gs : nullptr;
		if (sp && slope != made_slope) { // (stream order: the passes of the candidate before have read the planes by then)
			if (slope_planes == nullptr) return hipErrorInvalidValue;
			if ((e = launch_feature_slope(stream, feat_planes, W, H, slope, slope_planes)) != hipSuccess) return e;
			made_slope = slope;
		}
		double *f_a = cand_img + (size_t)i * stride, *f_b = f_a + 3u * N, *s_i = f_a + 6u * N;
		for (int pass = 0; pass < 2; pass++) { // launch_denoise_dual's two passes
			const double *Pw = pass == 0 ? PB : PA, *Uv = pass == 0 ? PA : PB;
			double *fout = pass == 0 ? f_a : f_b;
			const DualGain gn{pass == 0 ? g_a : g_b};
			e = tw == 32u ? launch_dual_pass_gain<32>(stream, grid, lds, Pw, Uv, W, H, ri, fi, k2, c.alpha, fout, gp, sp, gn)
			              : launch_dual_pass_gain<24>(stream, grid, lds, Pw, Uv, W, H, ri, fi, k2, c.alpha, fout, gp, sp, gn);
			if (e != hipSuccess) return e;
		}
		hipLaunchKernelGGL(dual_sure_kernel, dim3(blocks), dim3(256), 0, stream, planes, f_a, f_b, g_a, g_b, n_a, n_b, N, s_i);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	hipLaunchKernelGGL(dual_winner_kernel, dim3(blocks), dim3(256), 0, stream, cand_img + 6u * N, stride, n_cands, planes, W, H, (int)sure_window, win_img);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL(dual_blend_kernel, dim3(blocks), dim3(256), 0, stream, accum_a, accum_b, n_a, n_b, planes, cand_img, stride, n_cands, win_img, W, H, (int)select_window,
	                   out, err, sure, win);
	return hipGetLastError();
}

// One workgroup per rect.  Thread t adds the err of the rect's pixels t, t + 256, t + 512, ... (row-major within the rect) in that order; the 256
// partial sums are then added pairwise, halving: first lanes 32 apart within each wave, down to neighbours, then the four waves' sums as
// (w0 + w1) + (w2 + w3).  A NaN err anywhere in the rect makes the result +inf.
__global__ __launch_bounds__(256) void tile_error_dual_kernel(const double *__restrict__ err, const rmd_tile_rect *__restrict__ rects, uint32_t W,
                                                               double *__restrict__ out) {
	const rmd_tile_rect r = rects[blockIdx.x];
	const uint64_t n_px = (uint64_t)r.width * r.height;
	double s = 0.0;
	uint32_t bad = 0u;
	for (uint64_t i = threadIdx.x; i < n_px; i += 256u) {
		const double e = err[rect_pixel(r, i, W)];
		if (e == e) s = s + e;
		else bad = 1u;
	}
	for (int off = 32; off > 0; off >>= 1) s = s + __shfl_xor(s, off, 64), bad |= __shfl_xor(bad, off, 64);
	__shared__ double wave_sum[4];
	__shared__ uint32_t wave_bad[4];
	if ((threadIdx.x & 63u) == 0u) wave_sum[threadIdx.x >> 6] = s, wave_bad[threadIdx.x >> 6] = bad;
	__syncthreads();
	if (threadIdx.x == 0u) {
		const double total = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
		const bool any_bad = (wave_bad[0] | wave_bad[1] | wave_bad[2] | wave_bad[3]) != 0u;
		out[blockIdx.x] = any_bad ? __builtin_inf() : (n_px ? __builtin_sqrt(total / (double)n_px) : 0.0);
	}
}
hipError_t launch_tile_error_dual(hipStream_t stream, const double *err, const rmd_tile_rect *rects, uint32_t n_rects, uint32_t W, double *out) {
	if (n_rects == 0) return hipSuccess;
	hipLaunchKernelGGL(tile_error_dual_kernel, dim3(n_rects), dim3(256), 0, stream, err, rects, W, out);
	return hipGetLastError();
}

} // namespace rmd
