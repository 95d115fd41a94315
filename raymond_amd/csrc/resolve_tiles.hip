// The output stage over tile rectangles (rmd_resolve_tonemap_tiles; include/raymond_hip.h states the definition, DESIGN.md section 20 the structure).
// A translation unit of its own: no other unit's code objects change.
//
// resolve_tiles_kernel<DUAL> — one workgroup per ResolveRun (resolve_tiles_host.hpp): at most 1024 consecutive packed pixels of ONE rect, inside one
//                              1024-pixel chunk of the packed output.  A lane owns one GROUP of four packed pixels — bytes 12 g .. 12 g + 11 of the
//                              output, three whole dwords — clipped to the run: it reads each pixel's 24 bytes (48 with DUAL: the second sum buffer,
//                              added in one rounded addition) from the frame, evaluates tonemap_kernel's arithmetic word for word, and writes the group
//                              as three dword stores; a group the run's ends cut (a rect boundary inside it) is written byte by byte, so that two
//                              workgroups never write the same byte and nobody reads the output back.  No LDS, no barrier: the kernel streams.
//                              Flagged pixels (launch.hpp: kTonemapGuard) go into a list as PACKED indices, from which the host finds rect and frame
//                              position again (resolve_locate).
// The run's eight words are the same for every lane of the workgroup: scalar loads.  f64 throughout, built with -ffp-contract=off like the rest.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "resolve_tiles_host.hpp"

namespace rmd {

template <bool DUAL>
__global__ __launch_bounds__(256) void resolve_tiles_kernel(const double *__restrict__ accum, const double *__restrict__ accum2, uint32_t W,
                                                             const ResolveRun *__restrict__ runs, double exposure, double inv_gamma,
                                                             uint8_t *__restrict__ rgb8, uint32_t *__restrict__ flagged, uint32_t *__restrict__ n_flagged) {
	const ResolveRun r = runs[blockIdx.x];
	// 64-bit: the last group of a frame of 2^32 - 1 pixels ends past 2^32
	const uint64_t group = (uint64_t)(r.start / kResolveGroup) + threadIdx.x, run_end = (uint64_t)r.start + r.n;
	const uint64_t lo = group * kResolveGroup > r.start ? group * kResolveGroup : r.start;
	const uint64_t hi = (group + 1u) * kResolveGroup < run_end ? (group + 1u) * kResolveGroup : run_end;
	if (lo >= hi) return;
	const double sc = (double)r.samples;
	uint32_t word[3] = {0u, 0u, 0u};
#pragma unroll
	for (uint32_t k = 0; k < kResolveGroup; k++) {
		const uint64_t p = group * kResolveGroup + k;
		if (p < lo || p >= hi) continue;
		const uint32_t local = r.local + (uint32_t)(p - r.start);
		const uint32_t x = local % r.width, y = local / r.width;
		const size_t i = ((size_t)(r.left + x) + (size_t)(r.top + y) * W) * 3;
		double v[3];
		bool ok = true, flag = false;
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const double s = DUAL ? accum[i + c] + accum2[i + c] : accum[i + c];
			const double px = s / sc; // TaskHandle::await, src/trace.rs:95
			const double arg = px * -1.0 * exposure;
			double tm = 1.0 - exp(arg);
			tm = pow(tm, inv_gamma);
			v[c] = tm * 255.0;
			ok = ok && (v[c] > -1.0 && v[c] < 256.0);
			const double rn = __builtin_rint(v[c]);
			flag = flag || (rn >= 1.0 && __builtin_fabs(v[c] - rn) < kTonemapGuard && !(arg <= -40.0));
		}
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const uint32_t b = k * 3u + (uint32_t)c, byte = ok ? (uint32_t)(uint8_t)v[c] : 0u;
			word[b >> 2] |= byte << ((b & 3u) * 8u);
		}
		if (flag) flagged[atomicAdd(n_flagged, 1u)] = (uint32_t)p; // the list has room for every packed pixel
	}
	if (hi - lo == kResolveGroup) {
		uint32_t *out = reinterpret_cast<uint32_t *>(rgb8) + group * 3u; // rgb8 is a hipMalloc block's start: 12 g is a multiple of 4
		out[0] = word[0], out[1] = word[1], out[2] = word[2];
	} else {
#pragma unroll
		for (uint32_t k = 0; k < kResolveGroup; k++) {
			const uint64_t p = group * kResolveGroup + k;
			if (p < lo || p >= hi) continue;
#pragma unroll
			for (uint32_t c = 0; c < 3u; c++) {
				const uint32_t b = k * 3u + c;
				rgb8[p * 3u + c] = (uint8_t)(word[b >> 2] >> ((b & 3u) * 8u));
			}
		}
	}
}

hipError_t launch_resolve_tiles(hipStream_t stream, const double *accum, const double *accum2, uint32_t W, const ResolveRun *runs, uint32_t n_runs,
                                double exposure, double inv_gamma, uint8_t *rgb8, uint32_t *flagged, uint32_t *n_flagged) {
	if (n_runs == 0) return hipSuccess;
	if (accum2) hipLaunchKernelGGL(resolve_tiles_kernel<true>, dim3(n_runs), dim3(256), 0, stream, accum, accum2, W, runs, exposure, inv_gamma, rgb8, flagged, n_flagged);
	else hipLaunchKernelGGL(resolve_tiles_kernel<false>, dim3(n_runs), dim3(256), 0, stream, accum, accum2, W, runs, exposure, inv_gamma, rgb8, flagged, n_flagged);
	return hipGetLastError();
}

} // namespace rmd
