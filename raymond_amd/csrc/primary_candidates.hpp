// Which objects the primary rays of one 8x8 wave tile can hit: the predicate the role-sorted spheres kernel (render_kernel.hpp:
// render_wave_sorted) evaluates once per work item, and the host-only probe rmd_probe_primary_candidates evaluates for the tests
// (tests/test_primary_candidates.py).  One source for both: plain binary64 operations, compiled without contraction on either side.
//
// A generation trip of that kernel carries 64 pinhole rays from ONE camera position through ONE tile (device_core.hpp: primary_ray —
// ro = cam_pos, rd = normalize(px, py, 1), no rotation) and runs them against every object in branch-free code that all lanes execute in full.
// For most tiles the outcome of most of those tests follows from the tile, the camera and the scene alone:
//   * a sphere whose distance from every line of the tile's bounding cone exceeds its radius registers no hit (sphere_test_flat: `!(p > r2)`);
//   * of the room's (up to) three axis pairs (scene_split.hpp: axis_pair_test) one is nearer than the other two for every ray of the tile, so
//     the other two never hold the closest hit.
// The host turns this on (RenderParams::primary_cull) only for a scene of regular parameters (api_scene.cpp: rmd_scene::regular — every coordinate and
// radius finite and tame) without a grid, a launch without the thin lens (whose rays leave from the lens disc, not from cam_pos), and a camera
// whose position, tan_half_fov, aspect, width and height are finite, the last four positive.  Every comparison below is written so that a NaN
// keeps the object.
//
// THE TILE'S RAYS.  Lane (lx, ly) of tile (x0, y0, w, h) has xi = x0 + lx, and x + 0.5 = xi + u0 with u0 in [0, 1): in binary64 the sum can
// round up to xi + 1, so the pixel coordinate lies in the CLOSED interval [x0, x0 + w], likewise y.  sx = (x + 0.5) / width, px = (2 sx - 1) *
// tan_half_fov * aspect, py = (1 - 2 sy) * tan_half_fov: five roundings, a relative error below 4 eps of |px| + tan_half_fov * aspect.  The
// intervals [px_lo, px_hi] x [py_lo, py_hi] computed here from the tile's edges are widened on every side by kWiden = 1e-9 of tan_half_fov * aspect
// (of tan_half_fov for py): four million times that error.  The tile's rays are all directions (px, py, 1) inside that rectangle.
//
// SPHERE.  Let a = normalize(rectangle's centre, 1) and theta the largest angle between a and a corner (px, py, 1): the directions within theta
// of a meet the plane z = 1 in a convex region (theta < 90 degrees), so the whole rectangle lies inside that cone when its corners do.  With
// v = centre - cam_pos, L = |v| and phi the angle between v and a, every ray of the tile makes an angle in [phi - theta, phi + theta] with v.  If
// phi + theta < 90 degrees the sine is monotonic over that interval and the distance of the centre from the ray's LINE is at least
//     D = L sin(phi - theta) = |v x a| cos(theta) - (v . a) sin(theta).
// (A sphere to the side of or behind the camera fails phi + theta < 90 degrees and keeps its bit: it need not be recognised.)  The bit is
// cleared only if D > |radius| + margin.  The margin: sphere_test_flat forms c = centre - ro (relative error eps / 2 per component), t = c . rd
// (rd's components carry <= 3 eps each: |rd|^2 = 1 +- 6 eps and the direction is off by <= 3 eps), q = c - t rd and p = q . q, r2 = radius^2.
// |q| differs from the true distance by at most (4 + 1 + 1) sqrt(3) eps L from the roundings of t, t rd and the subtraction, 6 eps L from
// |rd| != 1 and 3 eps L from rd's direction: below 20 eps L; the roundings of p and r2 add eps |q| and eps |radius| / 4.  With
// K = |v|_1 + |centre|_1 + |cam_pos|_1 + |radius| >= L + |radius| the computed `p > r2` therefore holds whenever the true distance exceeds
// |radius| + 24 eps K.  That bound is taken a HUNDREDFOLD and rounded up, margin = 3200 eps K (internal.hpp: triangle_sphere sets the precedent);
// the rounding of D itself (a dozen operations on values below K: < 32 eps K) disappears in it.  A camera inside or near the sphere has
// D <= L < |radius| + margin and never clears the bit.
//
// AXIS PAIRS.  axis_pair_test<k> registers, for a lane whose ray has |rd_k| > 1e-6, the wall the ray faces — normal -e_k (coordinate o_minus)
// for rd_k > 0, +e_k (o_plus) for rd_k < 0 — at t = num / |rd_k| with num = o_minus - ro_k resp. ro_k - o_plus, if t >= 0.  Required first:
// on EVERY paired axis the camera lies strictly inside the room, o_plus < cam_pos_k < o_minus, so every numerator is positive (and none is
// a zero: the general test's fall-back never runs).  With u = (px, py, 1) and rd = u / |u|, t = num |u| / |u_k|: the common factor |u| drops out
// of every comparison between pairs of the same ray.  Pair k is KEPT ALONE only if, over the whole rectangle,
//   (1) u_k keeps one sign (the z pair always: u_z = 1), so one definite wall is faced, and min |u_k| / max |u| > 2e-6: |rd_k| is above the
//       facing threshold 1e-6 by a factor of two against <= 3 eps of rounding;
//   (2) that wall's numerator is positive (the camera is inside): the hit registers with t >= 0;
//   (3) s_k = num_k / min |u_k|, an upper bound of t_k / |u|, stays below the lower bound s_j of every other pair j — the smaller, over the
//       walls pair j's rays can face, of that wall's num_j / max |u_j| on its side of zero — by kPairMargin: s_k (1 + 1e-9) < s_j.  A computed t carries a relative error below 4 eps (numerator eps / 2, rd_k
//       3 eps, quotient eps / 2) and these bounds a few eps more: a million times smaller than the margin.
// Then every ray of the tile registers pair k's hit, and whatever a skipped pair would have registered is strictly farther: it never wins
// lex_less, whatever the index order.  A lane that carries no ray (outside a ragged tile) computes something nobody reads, as before.  Unpaired
// planes, objects from 64 on and the spheres that are not cleared are tested as before.
#pragma once
#include <stdint.h>

#include "device_types.hpp"

#if defined(__HIP__)
#define RMD_HD __host__ __device__ inline
#else
#define RMD_HD inline
#endif

namespace rmd {

constexpr double kCullWiden = 1e-9;       // the tile's px / py intervals grow by this much of the image plane's half extent on every side
constexpr double kCullSphereMargin = 3200.0 * 2.220446049250313e-16; // x K: a hundred times the derived bound 24 eps K, rounded up (see above)
constexpr double kCullFacing = 2e-6;      // |rd_k| of the kept pair stays above twice axis_pair_test's facing threshold
constexpr double kCullPairMargin = 1e-9;  // the kept pair's farthest hit is nearer than any other pair's nearest by this relative margin

// The launch's camera terms the predicate reads (RenderParams' own values: the kernel passes its parameters, the probe make_params' result).
struct CullCamera {
	double pos[3];
	double width, height, aspect, tan_half_fov;
};
// The bounding rectangle of a tile's directions (px, py, 1) and its bounding cone.
struct TileCone {
	double lo[2], hi[2]; // px, py intervals, widened
	double a[3];         // the cone's axis (unit)
	double cos_t, sin_t; // its half angle
	double u_max;        // largest |(px, py, 1)| over the rectangle
	bool ok;             // every value above is finite (else nothing is dropped)
};
RMD_HD double cull_abs(double v) { return v < 0.0 ? -v : v; }
RMD_HD double cull_min(double a, double b) { return a < b ? a : b; }
RMD_HD double cull_max(double a, double b) { return a > b ? a : b; }

// (the camera test of the host: finite position, and tan_half_fov, aspect, width, height finite and positive)
RMD_HD bool cull_camera_ok(const CullCamera &c) {
	const double big = 1e150;
	bool ok = cull_abs(c.pos[0]) <= big && cull_abs(c.pos[1]) <= big && cull_abs(c.pos[2]) <= big;
	ok = ok && c.tan_half_fov > 0.0 && c.tan_half_fov <= big && c.aspect > 0.0 && c.aspect <= big;
	return ok && c.width > 0.0 && c.width <= big && c.height > 0.0 && c.height <= big;
}

RMD_HD TileCone primary_tile_cone(const CullCamera &c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
	TileCone T;
	const double ex = c.tan_half_fov * c.aspect, ey = c.tan_half_fov;
	const double pxa = (2.0 * ((double)x0 / c.width) - 1.0) * ex, pxb = (2.0 * ((double)(x0 + w) / c.width) - 1.0) * ex;
	const double pya = (1.0 - 2.0 * ((double)y0 / c.height)) * ey, pyb = (1.0 - 2.0 * ((double)(y0 + h) / c.height)) * ey;
	T.lo[0] = cull_min(pxa, pxb) - kCullWiden * ex, T.hi[0] = cull_max(pxa, pxb) + kCullWiden * ex;
	T.lo[1] = cull_min(pya, pyb) - kCullWiden * ey, T.hi[1] = cull_max(pya, pyb) + kCullWiden * ey;
	const double cx = 0.5 * (T.lo[0] + T.hi[0]), cy = 0.5 * (T.lo[1] + T.hi[1]);
	const double cl = __builtin_sqrt((cx * cx + cy * cy) + 1.0);
	T.a[0] = cx / cl, T.a[1] = cy / cl, T.a[2] = 1.0 / cl;
	double cos_t = 1.0, sin_t = 0.0, u_max = 1.0;
	for (int k = 0; k < 4; k++) {
		const double qx = (k & 1) ? T.hi[0] : T.lo[0], qy = (k & 2) ? T.hi[1] : T.lo[1];
		const double ql = __builtin_sqrt((qx * qx + qy * qy) + 1.0);
		const double dx = qx / ql, dy = qy / ql, dz = 1.0 / ql;
		const double cs = (T.a[0] * dx + T.a[1] * dy) + T.a[2] * dz;
		const double kx = T.a[1] * dz - T.a[2] * dy, ky = T.a[2] * dx - T.a[0] * dz, kz = T.a[0] * dy - T.a[1] * dx;
		const double sn = __builtin_sqrt((kx * kx + ky * ky) + kz * kz);
		cos_t = cull_min(cos_t, cs), sin_t = cull_max(sin_t, sn), u_max = cull_max(u_max, ql);
	}
	T.cos_t = cos_t, T.sin_t = sin_t, T.u_max = u_max;
	// (a cone of 45 degrees or more — a tile that is most of a very wide frame — drops nothing)
	T.ok = cos_t > 0.7072 && sin_t < 0.7072 && u_max < 1e150 && T.lo[0] > -1e150 && T.hi[0] < 1e150 && T.lo[1] > -1e150 && T.hi[1] < 1e150;
	return T;
}

// true: no primary ray of the tile registers a hit on this sphere (its bit in the GI trips' visit mask may be cleared)
RMD_HD bool primary_sphere_cleared(const TileCone &T, const CullCamera &c, const double centre[3], double radius) {
	if (!T.ok) return false;
	const double vx = centre[0] - c.pos[0], vy = centre[1] - c.pos[1], vz = centre[2] - c.pos[2];
	const double va = (vx * T.a[0] + vy * T.a[1]) + vz * T.a[2];
	const double kx = vy * T.a[2] - vz * T.a[1], ky = vz * T.a[0] - vx * T.a[2], kz = vx * T.a[1] - vy * T.a[0];
	const double vxa = __builtin_sqrt((kx * kx + ky * ky) + kz * kz);
	const double r = cull_abs(radius);
	const double K = ((cull_abs(vx) + cull_abs(vy)) + cull_abs(vz)) + ((cull_abs(centre[0]) + cull_abs(centre[1])) + cull_abs(centre[2])) +
	                 ((cull_abs(c.pos[0]) + cull_abs(c.pos[1])) + cull_abs(c.pos[2])) + r;
	const double margin = kCullSphereMargin * K;
	const bool in_front = va * T.cos_t - vxa * T.sin_t > margin; // L cos(phi + theta) > 0: phi + theta < 90 degrees
	const double D = vxa * T.cos_t - va * T.sin_t;               // L sin(phi - theta)
	return in_front && D > r + margin && K <= 1e150;
}

// The one axis pair that holds every ray's closest wall hit, if there is one: its axis k, and whether the rays face the wall with normal -e_k
// (u_k > 0 over the whole rectangle: coordinate o_minus, object idx_minus) or the one with normal +e_k.  false: no pair qualifies.
RMD_HD bool primary_pair_alone(const TileCone &T, const CullCamera &c, const AxisWalls walls[3], uint32_t axis_pairs, int &k_alone, bool &faces_minus) {
	if (!T.ok) return false;
	double s_lo[3], s_hi[3]; // per paired axis: lower bound of t / |u| of whatever the pair registers; upper bound if it qualifies to be kept (else -1)
	bool paired[3], minus[3];
#pragma unroll
	for (int k = 0; k < 3; k++) {
		paired[k] = ((axis_pairs >> (10 * k)) & 1023u) != 0u;
		s_lo[k] = 0.0, s_hi[k] = -1.0, minus[k] = false;
		if (!paired[k]) continue;
		const double num_plus = c.pos[k] - walls[k].o_plus, num_minus = walls[k].o_minus - c.pos[k];
		if (!(num_plus > 0.0 && num_minus > 0.0)) return false; // the camera is not strictly inside the room on this axis (or a NaN)
		const double lo = k < 2 ? T.lo[k] : 1.0, hi = k < 2 ? T.hi[k] : 1.0;
		// the nearest hit the pair can register: over the part of the interval that faces the -e_k wall (u_k > 0) and the part that faces the other
		double nearest = 1e300; // (num / max |u_k| of each part; a part that does not exist registers nothing)
		if (hi > 0.0) nearest = cull_min(nearest, num_minus / hi);
		if (lo < 0.0) nearest = cull_min(nearest, num_plus / -lo);
		s_lo[k] = nearest;
		if (!(s_lo[k] > 0.0)) return false;
		const bool pos = lo > 0.0, neg = hi < 0.0;
		if (pos || neg) {
			const double u_lo = pos ? lo : -hi;
			if (u_lo > kCullFacing * T.u_max) s_hi[k] = (pos ? num_minus : num_plus) / u_lo, minus[k] = pos;
		}
	}
	bool found = false; // (the first pair that qualifies; written without an early exit: the kernel keeps all of this in registers)
#pragma unroll
	for (int k = 0; k < 3; k++) {
		bool alone = paired[k] && s_hi[k] > 0.0 && !found;
#pragma unroll
		for (int j = 0; j < 3; j++)
			if (j != k && paired[j]) alone = alone && s_hi[k] * (1.0 + kCullPairMargin) < s_lo[j];
		if (alone) found = true, k_alone = k, faces_minus = minus[k];
	}
	return found;
}
// The 10-bit fields of `axis_pairs` that stay for the tile's primary rays: all of them, or the one pair that holds every ray's closest wall hit.
RMD_HD uint32_t primary_pairs_kept(const TileCone &T, const CullCamera &c, const AxisWalls walls[3], uint32_t axis_pairs) {
	int k = 0;
	bool faces_minus = false;
	return primary_pair_alone(T, c, walls, axis_pairs, k, faces_minus) ? axis_pairs & (1023u << (10 * k)) : axis_pairs;
}

// TILE CLASSES.  What the role-sorted spheres kernel knows of a work item's samples before it draws one of them (render_kernel.hpp:
// render_wave_sorted).  Admission: the candidate sets' own (RenderParams::primary_cull — a regular scene without a grid, no thin lens, a finite
// camera) and RenderParams::end_black_paths != 0; anything else is kTileGeneral and runs the general code.
//
// ONE WALL.  The tile's primary rays all end on one and the same wall when
//   (a) the scene has at most 64 objects and the candidate visit mask is EMPTY: every sphere among them is cleared (primary_sphere_cleared: it
//       registers no hit for any ray of the cone) and no other object has a turn in the object loop — an unpaired plane, a plane pair that is
//       not an axis pair and an object from 64 on all keep theirs, and make the tile general;
//   (b) primary_pair_alone holds for a pair k.  Its conditions are the ones a definite wall needs, with the margins derived above: (1) u_k keeps
//       one sign over the widened rectangle, so every ray faces the same wall of the pair — the one with normal -e_k for u_k > 0 —, and
//       |rd_k| >= min |u_k| / max |u| > 2e-6, twice axis_pair_test's facing threshold against <= 3 eps of rounding: the denominator test
//       `|rd_k| > 1e-6` passes in every lane; (2) the wall's numerator, the very subtraction axis_pair_test makes (o_minus - ro_k resp.
//       ro_k - o_plus, ro = cam_pos exactly), is positive: a subtraction's sign is exact, so t = num / |rd_k| > 0 >= 0 registers, and it is finite
//       (num <= 2e150, |rd_k| > 1e-6) and so beats the loop's initial kFMax; (3) every other pair's hit is strictly farther.
// Then Scene::intersect returns that wall's object for every ray of the tile, whatever its jitter: nothing else registers a hit, or a closer one.
//
// FROM THE WALL'S RECORD.  kTileEmitter when material_kind == 2: the sample is hadamard((1, 1, 1), colour) = the colour, bit for bit (1.0 * x = x
// for every finite x, and a regular scene's colours are finite), and no random number enters it.  kTileBlack when kObjBlackDiffuse is set and
// prob_d = lerp(0.5, 0, metalness) = 0.5 + metalness * (0 - 0.5) compares equal to 0.5 — then `lobe_bits < 2^21`, the classification's test, and
// bounce_is_diffuse (lobe_bits * 2^-22 < prob_d) are the same statement: a sample whose block 0 has lobe_bits < 2^21 is (0, 0, 0), any other is
// parked as a GGX hit.  Anything else: general.
// The classification ends such a hit only if finite_inputs holds (the normal's and the hit point's components sum to something finite).  Here it
// does: the wall's normal is +-e_k exactly, and frag = cam_pos + rd * t with |cam_pos_a| <= 1e150 (cull_camera_ok: part of the admission), |rd_a| <= 1 + 3 eps and
// 0 < t <= 2e150 / 1e-6: every component below 3e156.  The wall coordinates are tame (|o| <= 1e150: the scene is regular) and compared with
// the camera's in (2); a NaN there fails the comparison and the tile is general.
enum : uint32_t { kTileGeneral = 0u, kTileEmitter = 1u, kTileBlack = 2u };
constexpr uint32_t kTileClassShift = 30u; // the class rides in the two bits the three 10-bit pair fields leave free (render_kernel.hpp: item_candidates)
// The object every primary ray of the tile hits, or -1.  alone, faces_minus: primary_pair_alone's answer for the tile (one evaluation serves the
// candidate pairs and the class), pair: the kept pair's record (the kernel reads it where the scene keeps it: a copy of the three records indexed
// by k would live in scratch memory); `visit` is the tile's candidate visit mask (the launch's mask less the cleared spheres).
RMD_HD int primary_one_wall(bool alone, bool faces_minus, const AxisWalls &pair, unsigned long long visit, uint32_t n_objects) {
	return (alone && visit == 0ull && n_objects - 1u < 64u) ? // (1 .. 64 objects: a pair that is alone has two)
	       (int)(faces_minus ? pair.idx_minus : pair.idx_plus) : -1;
}
RMD_HD uint32_t primary_wall_class(uint32_t material_kind, uint32_t flags, double metalness);
// The whole composition, for the kernel (item_candidates) and the host probe alike: the class of a tile whose candidate visit mask is `visit` and
// whose pair test answered (alone, k_alone, faces_minus), and in `wall` the object every primary ray of a classed tile hits.  walls: the scene's three
// records where it keeps them; objs: its object table (the kernel's staged copy).
RMD_HD uint32_t primary_tile_class(bool alone, int k_alone, bool faces_minus, const AxisWalls *walls, unsigned long long visit, uint32_t n_objects, const DevObject *objs,
                                   uint32_t &wall);
RMD_HD uint32_t primary_wall_class(uint32_t material_kind, uint32_t flags, double metalness) {
	if (material_kind == 2u) return kTileEmitter;
	const double prob_d = 0.5 + metalness * (0.0 - 0.5); // device_core.hpp: lerp(0.5, 0.0, metal), bounce_is_diffuse's operand
	return ((flags & kObjBlackDiffuse) != 0u && prob_d == 0.5) ? kTileBlack : kTileGeneral;
}
RMD_HD uint32_t primary_tile_class(bool alone, int k_alone, bool faces_minus, const AxisWalls *walls, unsigned long long visit, uint32_t n_objects, const DevObject *objs,
                                   uint32_t &wall) {
	wall = 0u;
	const int w = primary_one_wall(alone, faces_minus, walls[alone ? k_alone : 0], visit, n_objects);
	if (w < 0) return kTileGeneral;
	const DevObject &o = objs[w];
	const uint32_t cls = primary_wall_class(o.material_kind, o.flags, o.metalness);
	if (cls != kTileGeneral) wall = (uint32_t)w;
	return cls;
}

} // namespace rmd
