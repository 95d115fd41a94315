"""The expected words of rmd_render_ao and the expected image of rmd_ao_resolve, composed from the oracle's entry points and numpy, after
include/raymond_hip.h and nothing else:

  sample_primary_rays -> OracleScene.scene_intersect -> first_hit_ref.hit_features (the normal N) -> block_uniforms of the sample's NEXT block (block 1
  for the pinhole; 1 + the lens' rounds otherwise, the rounds found by restating the rejection loop of oracle.cpp's generate_primary_ray_with_dof over
  blocks 1, 2, ... — the accepted round's start point must be the oracle ray's origin bit for bit) -> orc_onb, orc_cosine_hemisphere ->
  dir = normalize(from_cols(T, N, B) * l), origin = frag + N * 0.00001 -> OracleScene.scene_intersect again; occluded where it hits nearer than
  max_distance.

tests/test_ao_host.py holds this composition to the oracle's render path (orc_trace_sample's second vertex on diffuse hits that take the diffuse lobe).

VARIANTS are four wrong readings of the definition, for tests/test_ao_host.py to tell the restatement from:
  block0            block 0's uniforms (the pixel jitter's) reused for the bounce
  offset_along_dir  the ray's origin moved off the surface along dir instead of along N
  normal_first      N the first column of the frame instead of the middle one
  skip_no_ray       a sample without a ray skipped instead of counted in `none`
"""
import collections
import ctypes as C
import functools
import math

import numpy as np

import first_hit_ref as fr
import oracle_lib as O

WORDS, OCCLUDED, OPEN, NONE, SAMPLES = 4, 0, 1, 2, 3
VARIANTS = ("block0", "offset_along_dir", "normal_first", "skip_no_ray")
Samples = collections.namedtuple("Samples", "first occluded no_ray rays obj t sub rays2 obj2 t2")


def lens_rounds(cam, seed, use_dof, pix, samples, rays, ok):
    """-> (n,) the rounds the thin lens' rejection loop takes for each (pixel, sample): 0 for the pinhole (and for the lens with aperture_radius not
    > 0, which the oracle takes as the pinhole).  The loop is restated over blocks 1, 2, ...; where the sample has a ray, the accepted round's start
    point is the oracle ray's origin bit for bit."""
    n = len(pix)
    rounds = np.zeros(n, dtype=np.uint32)
    c = cam.pod()
    ap = float(c.aperture_radius)
    if not (use_dof and ap > 0.0):
        return rounds
    px, py, pz = (float(c.position[k]) for k in range(3))
    for i in range(n):
        start = (px, py, pz)
        for j in range(4096):
            u = O.block_uniforms(seed, [pix[i]], [samples[i]], [1 + j])[0]
            r1, r2 = u[0] * 2.0 - 1.0, u[1] * 2.0 - 1.0
            start = (px + r1 * ap, py + r2 * ap, pz)
            dx, dy, dz = px - start[0], py - start[1], pz - start[2]
            rounds[i] = j + 1
            if math.sqrt(dx * dx + dy * dy + dz * dz) < ap:
                break
        if ok[i]:
            assert np.array(start).tobytes() == np.ascontiguousarray(rays[i, :3]).tobytes(), "the restated lens loop leaves the oracle's: pixel %d sample %d" % (pix[i], samples[i])
    return rounds


def bounce_rays(N, frag, r1, r2, variant=None):
    """trace()'s diffuse branch for n hits: normals N (n, 3), points frag (n, 3), uniforms r1, r2 (n,) -> rays (n, 6)"""
    L = O.load()
    n = len(r1)
    N, r1, r2 = O.f64(N).reshape(n, 3), O.f64(r1), O.f64(r2)
    T, B, l, pdf = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    if n:
        L.orc_onb(n, O.ptr(N), O.ptr(T), O.ptr(B))
        L.orc_cosine_hemisphere(n, O.ptr(r1), O.ptr(r2), O.ptr(l), O.ptr(pdf))
    c0, c1, c2 = (N, T, B) if variant == "normal_first" else (T, N, B)
    with np.errstate(all="ignore"):
        v = (c0 * l[:, 0:1] + c1 * l[:, 1:2]) + c2 * l[:, 2:3]  # Matrix3::from_cols(c0, c1, c2) * l
        d = v * (1.0 / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]))[:, None]  # normalize_to(1.0)
        origin = frag + (d if variant == "offset_along_dir" else N) * 0.00001
    return np.concatenate([origin, d], axis=1)


def sample_ao(scene, osc, cam, seed, use_dof, xy, samples, max_distance, variant=None):
    """-> Samples of the (x, y, sample) triples: first (n,) bool, the sample has a first hit; occluded (n,) bool; no_ray; the primary rays and their
    hits; the bounce rays (NaN rows where there is no first hit) and their hits (obj2 -1, t2 NaN there)"""
    xy = np.ascontiguousarray(xy, dtype=np.uint32).reshape(-1, 2)
    samples = np.ascontiguousarray(samples, dtype=np.uint32)
    phi, obj, t, sub, ok, rays = fr.sample_features(scene, osc, cam, seed, use_dof, xy, samples)
    pix = xy[:, 1] * cam.backbuffer_width + xy[:, 0]
    first = obj >= 0
    n = len(pix)
    rays2, obj2, t2 = np.full((n, 6), np.nan), np.full(n, -1, dtype=np.int32), np.full(n, np.nan)
    if first.any():
        at = np.flatnonzero(first)
        block = np.zeros(len(at), dtype=np.uint32) if variant == "block0" else 1 + lens_rounds(cam, seed, use_dof, pix[at], samples[at], rays[at], ok[at])
        u = O.block_uniforms(seed, pix[at], samples[at], block)
        with np.errstate(all="ignore"):
            frag = rays[at, :3] + rays[at, 3:] * t[at, None]
        rays2[at] = bounce_rays(phi[at, 0:3], frag, u[:, 0], u[:, 1], variant)
        obj2[at], t2[at], _ = osc.scene_intersect(rays2[at])
    with np.errstate(all="ignore"):
        occluded = first & (obj2 >= 0) & (t2 < max_distance)
    return Samples(first, occluded, ok == 0, rays, obj, t, sub, rays2, obj2, t2)


def count(words, first, occluded, active=None):
    """One sample per record: words (N, 4) uint32, changed in place; first, occluded (N,) bool; active (N,) bool or None = all"""
    a = np.ones(len(words), dtype=bool) if active is None else active
    words[:, OCCLUDED] += (a & first & occluded).astype(np.uint32)
    words[:, OPEN] += (a & first & ~occluded).astype(np.uint32)
    words[:, NONE] += (a & ~first).astype(np.uint32)
    words[:, SAMPLES] += a.astype(np.uint32)


def words_from_samples(first, occluded, base=None, no_ray=None, variant=None):
    """first, occluded (spp, H, W) bool -> (H, W, 4) uint32: the records after the samples in order, from `base` (H, W, 4) or zero"""
    spp, H, W = first.shape
    words = np.zeros((H * W, WORDS), dtype=np.uint32) if base is None else np.ascontiguousarray(base, dtype=np.uint32).reshape(H * W, WORDS).copy()
    for s in range(spp):
        active = ~np.asarray(no_ray[s], dtype=bool).reshape(-1) if variant == "skip_no_ray" and no_ray is not None else None
        count(words, first[s].reshape(-1), occluded[s].reshape(-1), active)
    return words.reshape(H, W, WORDS)


def resolve(words, empty_value=1.0):
    """(..., 4) words -> ((...) float64 open / (open + occluded), empty_value where the sum is 0; the number of such pixels)"""
    words = np.asarray(words, dtype=np.uint32)
    den = words[..., OPEN].astype(np.uint64) + words[..., OCCLUDED].astype(np.uint64)
    with np.errstate(all="ignore"):
        out = np.where(den == 0, np.float64(empty_value), words[..., OPEN].astype(np.float64) / den.astype(np.float64))
    return out, int((den == 0).sum())


def frame_samples(scene, cam, seed, spp, begin, use_dof, max_distance, variant=None):
    """-> Samples with every field shaped (spp, H, W[, k]): the frame's samples begin .. begin + spp - 1"""
    W, H = cam.backbuffer_width, cam.backbuffer_height
    osc = O.OracleScene(scene)
    xy, pix = fr.pixel_grid(W, H)
    per = [sample_ao(scene, osc, cam, seed, use_dof, xy, np.full(len(pix), s, dtype=np.uint32), max_distance, variant) for s in range(begin, begin + spp)]
    return Samples(*[np.stack([np.asarray(p[k]).reshape((H, W) + np.asarray(p[k]).shape[1:]) for p in per]) for k in range(len(Samples._fields))])


def frame_words(scene, cam, seed, spp, begin, use_dof, max_distance, variant=None, base=None):
    S = frame_samples(scene, cam, seed, spp, begin, use_dof, max_distance, variant)
    return words_from_samples(S.first, S.occluded, base=base, no_ray=S.no_ray, variant=variant)


# ---------------------------------------------------------------- the feature cases (tests/first_hit_ref.py) as AO cases
# max_distance is 1.0 unless the case, at 1.0, holds more than 3 pixels with a fragile sample (fragile_pixels below); such a case takes 0.5 or 2.0
# and is listed here.  tests/test_ao_host.py asserts the cap for every case at its distance.
DISTANCES = {}


def case_distance(key):
    return DISTANCES.get(key, 1.0)


# The frames that hold more than 3 pixels with a fragile sample, by feature_key_id, with the number measured on the CPU oracle (the same at 0.5, 1.0
# and 2.0): every one through fragile FIRST hits alone — tied walls, spheres or grids, a camera on a wall —, which no max_distance moves; by the two
# outcome rules each holds 0 such pixels.  tests/test_ao_host.py asserts the number as the frame's upper bound, and the full cap of 3 for every other frame.
OVER_CAP = {
    "duplicate_walls-0": 541, "duplicate_walls-1": 850, "camera_on_walls-0": 480, "camera_on_walls-1": 480, "camera_on_walls-2": 480,
    "camera_on_walls-3": 480, "camera_on_walls-5": 960, "camera_on_walls-6": 480, "camera_on_walls-7": 480, "coincident_spheres-0": 77,
    "coincident_spheres-1": 61, "coincident_spheres-0-lens": 89, "coincident_spheres-1-lens": 64, "shared_grid-0": 207, "shared_grid-1": 200,
    "shared_grid-2": 224, "shared_grid-3": 197, "shared_grid-0-lens": 264, "shared_grid-2-lens": 272, "camera_in_box-2": 10,
    "camera_on_wall_with_mesh-0": 594, "camera_on_wall_with_mesh-1": 616, "camera_on_wall_with_mesh-2": 594, "camera_on_wall_with_mesh-3": 616,
    "shared_grid-0-focal-1e6": 346, "shared_grid-0-aperture-1e-9": 161, "shared_grid-0-aperture-4": 562, "shared_grid-0-aperture-zero": 161,
}

# ... and the distance at its ends, on a scene without walls and in a closed room: +inf is "any hit", at 1e-3 only corners occlude
OPEN_SCENE = ("mesh", "open_scene", 0, False, None)
ROOM = ("spheres", "shuffled_room", 0, False, None)
EXTRA_DISTANCES = ((OPEN_SCENE, float("inf")), (ROOM, float("inf")), (ROOM, 1e-3))


@functools.lru_cache(maxsize=None)
def reference(key, max_distance=None):
    """the restatement's samples and words of a feature case at max_distance (None: the case's own): computed once per process, shared, read-only"""
    fc = fr.feature_case(key)
    D = case_distance(key) if max_distance is None else max_distance
    S = frame_samples(fc.scene, fc.cam, fc.seed, fc.spp, fc.begin, fc.use_dof, D)
    words = words_from_samples(S.first, S.occluded)
    for a in tuple(S) + (words,):
        a.setflags(write=False)
    return S, words


# ---------------------------------------------------------------- fragile samples: where a device may legitimately count another outcome
def moved_rays(rays):
    """first_hit_ref.fragile_hit's twelve moves of each of (n, 6) rays: each direction component and each origin component by +-1e-9 -> (n * 12, 6),
    a ray's twelve in a row"""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    moved = []
    with np.errstate(all="ignore"):
        for k in range(3):
            for sign in (-1.0, 1.0):
                d = rays[:, 3:].copy()
                d[:, k] += sign * 1e-9
                moved.append(np.concatenate([rays[:, :3], d / np.sqrt((d * d).sum(axis=1))[:, None]], axis=1))
                o = rays[:, :3].copy()
                o[:, k] += sign * 1e-9 * np.maximum(1.0, np.abs(o).max(axis=1))
                moved.append(np.concatenate([o, rays[:, 3:]], axis=1))
    return np.ascontiguousarray(np.stack(moved, axis=1).reshape(-1, 6))


def outcome_fragile(osc, rays2, obj2, t2, max_distance):
    """(n, 6) bounce rays with their hits -> (n,) bool: |t2 - max_distance| <= 1e-9 max_distance, or the occluded / open outcome flips under one of
    the twelve moves.  Rows without a ray (NaN) are False."""
    n = len(rays2)
    out = np.zeros(n, dtype=bool)
    have = ~np.isnan(rays2).any(axis=1)
    if not have.any():
        return out
    at = np.flatnonzero(have)
    with np.errstate(all="ignore"):
        occ = (obj2[at] >= 0) & (t2[at] < max_distance)
        near = (obj2[at] >= 0) & np.isfinite(max_distance) & (np.abs(t2[at] - max_distance) <= 1e-9 * max_distance)
        moved = moved_rays(rays2[at])
        o, t, _ = osc.scene_intersect(moved)
        flips = (((o >= 0) & (t < max_distance)).reshape(len(at), 12) != occ[:, None]).any(axis=1)
    out[at] = near | flips
    return out


def first_hit_fragile(scene, osc, rays, obj, t, sub, no_ray):
    """first_hit_ref.fragile_hit over (n, 6) primary rays, vectorised: grazing (the oracle's answer changes under one of the twelve moves) for every
    ray at once; tied (another candidate within 1e-9 relative of the hit) object by object for planes and spheres, ray by ray for a grid's triangles
    -> (n,) bool.  A sample without a ray (no_ray) has no first hit to be fragile; rows with a NaN are skipped."""
    L = O.load()
    n = len(rays)
    out = np.zeros(n, dtype=bool)
    ok = ~np.isnan(rays).any(axis=1) & ~np.asarray(no_ray, dtype=bool)
    at = np.flatnonzero(ok)
    if len(at):
        with np.errstate(all="ignore"):
            moved = moved_rays(rays[at])
        o2, _, s2 = osc.scene_intersect(moved)
        o2, s2 = o2.reshape(len(at), 12), s2.reshape(len(at), 12)
        out[at] = ((o2 != obj[at, None]) | ((o2 >= 0) & (s2 != sub[at, None]))).any(axis=1)
    hit = np.flatnonzero(ok & (obj >= 0) & ~out)
    if not len(hit):
        return out
    objs, _, descs, _, _keep = scene.flatten()
    R, T = np.ascontiguousarray(rays[hit]), t[hit]
    k = len(hit)
    tied = np.zeros(k, dtype=bool)
    for i, o in enumerate(objs):
        if o.geometry_kind == 2:
            g = descs[o.grid_index]
            m = int(g.n_tris)
            tp = np.ascontiguousarray(np.ctypeslib.as_array(C.cast(g.tri_pos, C.POINTER(C.c_double)), (m, 9)))
            h, tt = np.zeros(m, dtype=np.int32), np.zeros(m)
            for j in range(k):
                rr = np.ascontiguousarray(np.tile(R[j], (m, 1)))
                L.orc_triangle_intersect(m, O.ptr(tp), O.ptr(rr), O.ptr(h), O.ptr(tt))
                c = h != 0
                if obj[hit[j]] == i:
                    c[sub[hit[j]]] = False
                with np.errstate(all="ignore"):
                    tied[j] |= bool((c & (np.abs(tt - T[j]) <= 1e-9 * np.maximum(np.abs(T[j]), np.abs(tt)))).any())
            continue
        h, tt = np.zeros(k, dtype=np.int32), np.zeros(k)
        if o.geometry_kind == 0:
            prim = np.ascontiguousarray(np.tile(np.array(list(o.origin) + list(o.normal)), (k, 1)))
            L.orc_plane_intersect(k, O.ptr(prim), O.ptr(R), O.ptr(h), O.ptr(tt))
        else:
            prim = np.ascontiguousarray(np.tile(np.array(list(o.origin) + [o.radius]), (k, 1)))
            L.orc_sphere_intersect(k, O.ptr(prim), O.ptr(R), O.ptr(h), O.ptr(tt))
        with np.errstate(all="ignore"):
            tied |= (h != 0) & (obj[hit] != i) & (np.abs(tt - T) <= 1e-9 * np.maximum(np.abs(T), np.abs(tt)))
    out[hit] |= tied
    return out


def fragile_sample(scene, osc, S, max_distance):
    """One sample as a Samples of 1-element arrays -> why a device may count it otherwise: "first hit: tied / grazing", "near max_distance",
    "outcome flips", or None"""
    why = None if S.no_ray[0] else fr.fragile_hit(scene, osc, S.rays[0], S.obj[0], S.t[0], S.sub[0])  # (without a ray there is no first hit to be fragile)
    if why is not None:
        return "first hit: " + why
    if not S.first[0]:
        return None
    with np.errstate(all="ignore"):
        if S.obj2[0] >= 0 and np.isfinite(max_distance) and abs(S.t2[0] - max_distance) <= 1e-9 * max_distance:
            return "near max_distance"
    return "outcome flips" if outcome_fragile(osc, S.rays2[:1], S.obj2[:1], S.t2[:1], max_distance)[0] else None


def fragile_pixels(scene, S, max_distance):
    """frame Samples (spp, H, W, ...) -> (H, W) bool, (H, W) bool: the pixels holding a fragile sample, and those holding one by the outcome rules alone
    (near max_distance, or the outcome flips): the part of the definition that max_distance moves"""
    osc = O.OracleScene(scene)
    spp, H, W = S.first.shape
    flat = lambda a: np.ascontiguousarray(a).reshape((spp * H * W,) + a.shape[3:])
    first = first_hit_fragile(scene, osc, flat(S.rays), flat(S.obj), flat(S.t), flat(S.sub), flat(S.no_ray))
    outcome = outcome_fragile(osc, flat(S.rays2), flat(S.obj2), flat(S.t2), max_distance)
    return (first | outcome).reshape(spp, H, W).any(axis=0), outcome.reshape(spp, H, W).any(axis=0)


def random_records(rng, n):
    """n records for the resolve: all zero, only `none`, open alone, occluded alone, both, counts up to 2^32 - 1 whose sum passes 2^32 (records need not
    be reachable by the rule: the resolve is defined on the words)"""
    words = np.zeros((n, WORDS), dtype=np.uint32)
    kind = rng.integers(0, 7, n)
    small = rng.integers(1, 64, (n, 3)).astype(np.uint32)
    big = rng.integers(0x80000000, 0xFFFFFFFF, (n, 3), dtype=np.uint64, endpoint=True).astype(np.uint32)
    for k, cols in ((1, (NONE,)), (2, (OPEN,)), (3, (OCCLUDED,)), (4, (OCCLUDED, OPEN)), (5, (OCCLUDED, OPEN, NONE))):
        for c in cols:
            words[kind == k, c] = small[kind == k, c]
    for c in (OCCLUDED, OPEN, NONE):
        words[kind == 6, c] = big[kind == 6, c]
    words[:, SAMPLES] = words[:, OCCLUDED] + words[:, OPEN] + words[:, NONE]  # (uint32: wraps)
    return words
