// What rmd_despike_dual adds to the rule of rmd_despike (include/raymond_hip.h states the definition): the merge of the two halves, the dual validity and
// what a half takes from its donor.  Everything else — Y, V, the order of the others, the donor, the spike test, the scaled copy — is despike_rule.hpp's,
// unchanged.  The kernel (despike_dual.hip), the C++ mirror (raymond_amd/host) and tests/despike_dual_rule_main.cpp all read these lines.  Built without
// contraction (-ffp-contract=off) wherever it is built.
#pragma once
#include <stdint.h>

#include "despike_rule.hpp"

namespace rmd {

// The merged pixel: each of its six sums is ONE rounded addition of the halves' (rmd_luminance_histogram_tiles's rule for its second buffer)
RMD_LUMA_HD inline void despike_dual_merge(const double sa[3], const double qa[3], const double sb[3], const double qb[3], double s[3], double q[3]) {
	for (int c = 0; c < 3; c++) s[c] = sa[c] + sb[c], q[c] = qa[c] + qb[c];
}

// Valid: both halves hold a sample and the six MERGED sums are finite.  Finite merged sums imply finite halves; two finite halves whose sum overflows are
// not valid.  A pixel with an empty half is never a spike and never a donor: the scaled copy divides by the donor's half count
RMD_LUMA_HD inline bool despike_dual_valid(const double s[3], const double q[3], uint32_t n_a, uint32_t n_b) {
	return n_a >= 1u && n_b >= 1u && despike_finite(s[0]) && despike_finite(s[1]) && despike_finite(s[2]) && despike_finite(q[0]) && despike_finite(q[1]) &&
	       despike_finite(q[2]);
}

// Y and V of the merged pixel at n_a + n_b (the caller holds the sum below 2^32); false (and nothing written) for a pixel that is not valid.  A valid
// pixel's merged count is >= 2, so despike_pixel's own validity holds and its Y and V are rmd_despike's on (S, Q, n)
RMD_LUMA_HD inline bool despike_dual_pixel(const double sa[3], const double qa[3], uint32_t n_a, const double sb[3], const double qb[3], uint32_t n_b, double &Y,
                                           double &V) {
	double s[3], q[3];
	despike_dual_merge(sa, qa, sb, qb, s, q);
	if (!despike_dual_valid(s, q, n_a, n_b)) return false;
	return despike_pixel(s, q, n_a + n_b, Y, V);
}

// What half h of a spike takes of one of the donor's half-h sums: the donor's bits at equal half counts, else the donor's per-sample moment at the
// spike's own half count.  Both counts are >= 1: spike and donor are valid
RMD_LUMA_HD inline double despike_dual_take(double donor_half_sum, uint32_t n_donor_half, uint32_t n_p_half) {
	return n_p_half == n_donor_half ? donor_half_sum : despike_scaled(donor_half_sum, n_donor_half, n_p_half);
}

} // namespace rmd
