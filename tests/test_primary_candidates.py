"""The candidate sets of the spheres kernel's generation trips (raymond_amd/csrc/primary_candidates.hpp), held to the oracle on the CPU.

For the primary rays of one 8x8 wave tile the kernel leaves out the spheres no ray of the tile can hit and the axis pairs that cannot hold the
closest hit.  The host-only probe rmd_probe_primary_candidates evaluates the very function the kernel calls; this test sends the oracle's own
primary rays (orc_primary_ray) through the oracle's Scene::intersect (orc_scene_intersect) — the tile's corners, its edge mid-points, the
jitter extremes u = 0 and u = 1 - 2^-53 and 64 random jitters — and asserts, for every tile,
  * a sphere whose bit was cleared is never the hit object,
  * the closest object and its distance over the candidate set (the oracle on the scene WITHOUT the dropped objects) equal the oracle's on
    the whole scene, bit for bit,
over a few hundred seeded cameras (field of view, aspect, frame size, position inside and outside the room, near and inside spheres), rooms
and up to 64 spheres (and a few more: objects from 64 on are never dropped).  Nothing is dropped under the thin lens, in a scene outside the
regular parameter class, for a non-finite camera, or with RMD_TUNE_AXIS_PAIRS at 1 or 2.  On the benchmark frame (C2) at least 85 % of the
wave tiles are free of both spheres and at least 95 % keep one axis pair: the test cannot pass by never dropping anything."""
import ctypes as C

import numpy as np
import pytest

from raymond_amd import probe, scenes
from raymond_amd.scene import CameraSettings, Material, Object, Plane, Scene, Settings, Sphere, Transform

ONE_MINUS = 1.0 - 2.0**-53
N_RANDOM_JITTERS = 64


def wave_tiles(W, H):
    return np.array([(x, y, min(8, W - x), min(8, H - y)) for x in range(0, W, 8) for y in range(0, H, 8)], dtype=np.uint32)


def tile_rays(oracle, cam, tile, rng):
    """The oracle's primary rays of one tile: corners, edge mid-points, jitter extremes of corner and inner pixels, random jitters."""
    x0, y0, w, h = (int(v) for v in tile)
    x1, y1, xm, ym = x0 + w - 1, y0 + h - 1, x0 + (w - 1) // 2, y0 + (h - 1) // 2
    xy, u = [], []
    for px, ux in ((x0, 0.0), (xm, 0.5), (x1, ONE_MINUS)):  # corners and edge mid-points (and the centre)
        for py, uy in ((y0, 0.0), (ym, 0.5), (y1, ONE_MINUS)):
            xy.append((px, py)), u.append((ux, uy))
    for px in (x0, xm, x1):  # the jitter extremes of corner and inner pixels
        for py in (y0, ym, y1):
            for ux in (0.0, ONE_MINUS):
                for uy in (0.0, ONE_MINUS):
                    xy.append((px, py)), u.append((ux, uy))
    rx, ry = rng.integers(x0, x1 + 1, N_RANDOM_JITTERS), rng.integers(y0, y1 + 1, N_RANDOM_JITTERS)
    ru = np.floor(rng.random((N_RANDOM_JITTERS, 2)) * 2.0**53) * 2.0**-53
    xy = np.concatenate([np.array(xy, dtype=np.uint32), np.stack([rx, ry], axis=1).astype(np.uint32)])
    u = np.concatenate([np.array(u), ru])
    rays = np.zeros((xy.shape[0], 6))
    c = cam.pod()
    xy, u = np.ascontiguousarray(xy), np.ascontiguousarray(u)
    oracle.load().orc_primary_ray(xy.shape[0], C.byref(c), oracle.ptr(xy), oracle.ptr(u), oracle.ptr(rays))
    return rays


def pair_planes(scene, pairs_field):
    """The two planes of the axis pair a 10-bit field names: the later plane (field - 1) and the first earlier plane with the negated normal."""
    j = pairs_field - 1
    nj = scene.objects[j].geometry.normal
    for i in range(j):
        g = scene.objects[i].geometry
        if isinstance(g, Plane) and all(a == -b for a, b in zip(g.normal, nj)):
            return i, j
    raise AssertionError("axis pair without a partner")


def dropped_objects(scene, launch_visit, launch_pairs, visit, pairs):
    gone = [i for i in range(min(64, len(scene.objects))) if (launch_visit >> i) & 1 and not (int(visit) >> i) & 1]
    spheres = list(gone)
    for k in range(3):
        f = (launch_pairs >> (10 * k)) & 1023
        if f and not (int(pairs) >> (10 * k)) & 1023:
            gone.extend(pair_planes(scene, f))
    return spheres, sorted(gone)


def check_tiles(oracle, scene, cam, st, tiles, rng, stats):
    launch_visit, launch_pairs, on, visit, pairs = probe.primary_candidates(cam, st, scene, tiles)
    # whatever stays is part of what the launch visits; a pair's field stays whole or goes
    assert all(int(v) & ~launch_visit == 0 for v in visit)
    for p in pairs:
        for k in range(3):
            assert ((int(p) >> (10 * k)) & 1023) in (0, (launch_pairs >> (10 * k)) & 1023)
    full = oracle.OracleScene(scene)
    reduced = {}
    for tile, v, p in zip(tiles, visit, pairs):
        spheres, gone = dropped_objects(scene, launch_visit, launch_pairs, v, p)
        stats["tiles"] += 1
        stats["spheres_dropped"] += len(spheres)
        stats["pairs_dropped"] += (len(gone) - len(spheres)) // 2
        for i in spheres:
            assert isinstance(scene.objects[i].geometry, Sphere) and i < 64
        if not gone:
            continue
        assert on
        rays = tile_rays(oracle, cam, tile, rng)
        obj, t, _ = full.scene_intersect(rays)
        assert not np.isin(obj, spheres).any(), ("a dropped sphere is the hit object", tile, spheres)
        key = tuple(gone)
        if key not in reduced:
            keep = [i for i in range(len(scene.objects)) if i not in gone]
            sub = Scene()
            sub.objects = [scene.objects[i] for i in keep]
            reduced[key] = (oracle.OracleScene(sub), np.array(keep + [-1], dtype=np.int64))
        sub_scene, back = reduced[key]
        obj_c, t_c, _ = sub_scene.scene_intersect(rays)
        obj_c = back[obj_c]  # (-1 -> -1: the last entry)
        assert np.array_equal(obj_c, obj), ("the closest object over the candidate set differs", tile, gone)
        hit = obj >= 0
        assert np.array_equal(t_c[hit].view(np.uint64), t[hit].view(np.uint64)), ("the closest distance over the candidate set differs", tile, gone)
        stats["rays"] += rays.shape[0]
    return on, launch_visit, launch_pairs, visit, pairs


def random_room(rng, n_spheres, extra_planes=0):
    lo = -rng.uniform(0.5, 6.0, 3)
    hi = rng.uniform(0.5, 6.0, 3)
    mats = [Material.Diffuse((0.7, 0.7, 0.7), 0.5), Material.Emission((1.5, 1.5, 1.5)), Material.Diffuse((0.0, 0.0, 0.0), 0.3), Material.Metal((0.9, 0.8, 0.1), 0.1)]
    objs = []
    for k in range(3):
        e = [0.0, 0.0, 0.0]
        o_lo, o_hi = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        e[k], o_lo[k], o_hi[k] = 1.0, lo[k], hi[k]
        objs.append(Object(Plane(o_lo, e), mats[int(rng.integers(0, 4))]))
        objs.append(Object(Plane(o_hi, [-v for v in e]), mats[int(rng.integers(0, 4))]))
    for _ in range(extra_planes):  # unpaired, tilted: tested as before
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        objs.append(Object(Plane(rng.uniform(-3, 3, 3), n), mats[int(rng.integers(0, 4))]))
    for _ in range(n_spheres):
        c = rng.uniform(lo * 1.2, hi * 1.2)
        objs.append(Object(Sphere(c, rng.choice([0.02, 0.1, 0.3, 0.8, 2.0]) * rng.uniform(0.5, 1.5)), mats[int(rng.integers(0, 4))]))
    order = rng.permutation(len(objs))
    scene = Scene()
    scene.objects = [objs[i] for i in order]
    return scene, lo, hi


def random_camera(rng, scene, lo, hi, case):
    W, H = int(rng.integers(9, 97)), int(rng.integers(9, 97))
    if case % 7 == 0:
        W, H = int(rng.integers(100, 400)), int(rng.integers(9, 40))  # a wide strip: a large aspect
    fov = float(rng.choice([12.0, 35.0, 55.0, 90.0, 120.0, 150.0]) * rng.uniform(0.9, 1.1))
    kind = case % 5
    spheres = [o.geometry for o in scene.objects if isinstance(o.geometry, Sphere)]
    if kind == 0 or not spheres:
        pos = rng.uniform(lo * 0.95, hi * 0.95)  # inside the room
    elif kind == 1:
        pos = rng.uniform(lo * 2.0, hi * 2.0)  # anywhere, outside the room as well
    elif kind == 2:
        s = spheres[int(rng.integers(0, len(spheres)))]  # close to a sphere's surface, either side of it
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        pos = np.array(s.origin) + d * s.radius * float(rng.choice([0.5, 0.999999, 1.0, 1.000001, 1.05]))
    elif kind == 3:
        pos = np.array(spheres[int(rng.integers(0, len(spheres)))].origin)  # at a sphere's centre
    else:
        pos = rng.uniform(lo, hi)
        k = int(rng.integers(0, 3))
        pos[k] = (lo[k], hi[k])[int(rng.integers(0, 2))] * float(rng.choice([1.0, 1.0 - 1e-12, 1.0 + 1e-12]))  # on a wall, or a hair off it
    return CameraSettings(W, H, fov, Transform(tuple(float(v) for v in pos)))


def test_dropped_objects_are_never_hit_and_the_candidates_hold_the_closest_hit(oracle, product_lib):
    rng = np.random.default_rng(0xC0FFEE)
    stats = dict(tiles=0, rays=0, spheres_dropped=0, pairs_dropped=0)
    n_on = 0
    for case in range(300):
        n_spheres = int(rng.choice([0, 1, 2, 5, 20, 58, 64]))
        scene, lo, hi = random_room(rng, min(n_spheres, 58), extra_planes=int(rng.integers(0, 3)) if n_spheres < 58 else 0)
        assert len(scene.objects) <= 64
        cam = random_camera(rng, scene, lo, hi, case)
        st = Settings(cam, sample_count=1)
        tiles = wave_tiles(cam.backbuffer_width, cam.backbuffer_height)
        if len(tiles) > 24:
            tiles = tiles[rng.choice(len(tiles), 24, replace=False)]
        on, *_ = check_tiles(oracle, scene, cam, st, tiles, rng, stats)
        n_on += on
    print(stats, "cases with the candidate sets on:", n_on)
    assert n_on == 300
    assert stats["spheres_dropped"] > 10000 and stats["pairs_dropped"] > 1000 and stats["rays"] > 100000, stats


def test_objects_from_64_on_are_never_dropped(oracle, product_lib):
    rng = np.random.default_rng(7)
    scene, lo, hi = random_room(rng, 90)
    cam = CameraSettings(64, 48, 55.0, Transform((0.0, 0.0, 0.0)))
    stats = dict(tiles=0, rays=0, spheres_dropped=0, pairs_dropped=0)
    on, launch_visit, _, visit, _ = check_tiles(oracle, scene, cam, Settings(cam, sample_count=1), wave_tiles(64, 48), rng, stats)
    assert on and stats["spheres_dropped"] > 0
    # (the masks speak of objects 0 .. 63 only: the object loop visits every later one, and the comparison with the oracle above had them in)
    assert launch_visit < 2**64 and all(int(v) < 2**64 for v in visit)


def test_nothing_is_dropped_outside_the_conditions(product_lib):
    sc = scenes.reflective_spheres()
    W, H = 256, 144
    tiles = wave_tiles(W, H)
    cam = scenes.camera(W, H)
    st = Settings(cam, sample_count=1)

    def unchanged(cam, st, scene, tunable=0, expect_pairs=True):
        lv, lp, on, visit, pairs = probe.primary_candidates(cam, st, scene, tiles, tunable)
        assert not on
        assert (visit == np.uint64(lv)).all() and (pairs == np.uint32(lp)).all()
        assert (lp != 0) == expect_pairs
        return lv, lp

    lv, lp, on, visit, pairs = probe.primary_candidates(cam, st, sc, tiles)
    assert on and (visit != np.uint64(lv)).any() and (pairs != np.uint32(lp)).any()  # the same launch inside the conditions does drop
    # the thin lens
    cam_dof = scenes.camera(W, H, aperture_radius=0.05)
    unchanged(cam_dof, Settings(cam_dof, sample_count=1, use_dof=True), sc)
    # a scene outside the regular parameter class (roughness 0; a NaN colour; a sphere of radius 0): no axis pairs either
    for bad in (Object(Sphere((0.0, 0.0, 3.0), 0.3), Material.Metal((1.0, 1.0, 1.0), 0.0)),
                Object(Sphere((0.0, 0.0, 3.0), 0.3), Material.Diffuse((float("nan"), 0.0, 0.0), 0.5)),
                Object(Sphere((0.0, 0.0, 3.0), 0.0), Material.Diffuse((0.5, 0.5, 0.5), 0.5))):
        irregular = scenes.reflective_spheres()
        irregular.objects.append(bad)
        unchanged(cam, st, irregular, expect_pairs=False)
    # a camera that is not finite
    for pos in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 0.0, -float("inf"))):
        c = CameraSettings(W, H, 55.0, Transform(pos))
        unchanged(c, Settings(c, sample_count=1), sc)
    for fov in (0.0, float("nan"), -55.0):  # tan_half_fov zero, NaN, negative
        c = CameraSettings(W, H, fov, Transform((0.0, 0.0, 0.0)))
        unchanged(c, Settings(c, sample_count=1), sc)
    # the switch: RMD_TUNE_AXIS_PAIRS = 1 (no pairs, no candidate sets), 2 (pairs, no candidate sets)
    unchanged(cam, st, sc, tunable=1, expect_pairs=False)
    lv2, lp2 = unchanged(cam, st, sc, tunable=2)
    assert (lv2, lp2) == (lv, lp)


def test_the_benchmark_frame_is_mostly_freed(product_lib):
    sc = scenes.reflective_spheres()
    st = scenes.config_settings("C2")
    cam = st.camera_settings
    tiles = wave_tiles(cam.backbuffer_width, cam.backbuffer_height)
    assert len(tiles) == 32400
    lv, lp, on, visit, pairs = probe.primary_candidates(cam, st, sc, tiles)
    assert on and lv & 3 == 3  # the two spheres are objects 0 and 1
    free_of_both = float(((visit & np.uint64(3)) == 0).mean())
    n_pairs = sum(((pairs >> np.uint32(10 * k)) & np.uint32(1023)) != 0 for k in range(3))
    one_pair = float((n_pairs == 1).mean())
    print("C2: tiles free of sphere 0 %.2f %%, of sphere 1 %.2f %%, of both %.2f %%; one axis pair left %.2f %%" % (
        100 * float(((visit & np.uint64(1)) == 0).mean()), 100 * float(((visit & np.uint64(2)) == 0).mean()), 100 * free_of_both, 100 * one_pair))
    assert free_of_both >= 0.85
    assert one_pair >= 0.95


@pytest.mark.parametrize("name", ["C1", "C2"])
def test_benchmark_frames_against_the_oracle(oracle, product_lib, name):
    """The benchmark cameras themselves: every tile of C1, a seeded thousand of C2's."""
    rng = np.random.default_rng(11)
    sc = scenes.reflective_spheres()
    st = scenes.config_settings(name)
    cam = st.camera_settings
    tiles = wave_tiles(cam.backbuffer_width, cam.backbuffer_height)
    if len(tiles) > 1024:
        tiles = tiles[rng.choice(len(tiles), 1024, replace=False)]
    stats = dict(tiles=0, rays=0, spheres_dropped=0, pairs_dropped=0)
    on, *_ = check_tiles(oracle, sc, cam, st, tiles, rng, stats)
    assert on and stats["spheres_dropped"] > 0 and stats["pairs_dropped"] > 0, stats
