// The reference's 8-bit output stage for one pixel, with the host libm: what rmd_resolve_tonemap and rmd_resolve_tonemap_tiles (api_frame.cpp) give the
// pixels their kernels flag — those whose byte an ulp of the device's exp / pow could decide.  Needs only <cmath> and <stdint.h>, so that it can be run
// on the CPU by itself (tests/tonemap_host_main.cpp holds it to the oracle's restatement).
#pragma once
#include <stdint.h>

#include <cmath>

namespace rmd {

// sums: the pixel's three radiance sums; sc: its sample count; out: its three bytes — all 0 unless every channel can be cast
inline void tonemap_bytes(const double sums[3], double sc, double exposure, double inv_gamma, uint8_t out[3]) {
	double v[3];
	bool ok = true;
	for (int c = 0; c < 3; c++) {
		const double p = sums[c] / sc; // src/trace.rs:95
		double tm = 1.0 - std::exp(p * -1.0 * exposure); // cli_old/src/main.rs:165
		tm = std::pow(tm, inv_gamma);                    // :166
		v[c] = tm * 255.0;
		ok = ok && (v[c] > -1.0 && v[c] < 256.0); // :176 cast::<u8>()
	}
	for (int c = 0; c < 3; c++) out[c] = ok ? (uint8_t)v[c] : (uint8_t)0;
}

} // namespace rmd
