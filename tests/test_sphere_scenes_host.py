"""The adversarial scenes of tests/sphere_scenes.py on the CPU: are they a fair yardstick, and does each class reach what it is aimed at?

For every class and seed (and the thin-lens variants):
  * the oracle equals the second reading of the source (tests/second_reading.py) on a seeded handful of pixels and samples: every vertex
    sequence the same, the radiance bit for bit (NaN for NaN).  The scenes are built on exact ties — copied objects, a camera ON a wall — so this
    is what shows that the scenes do not split the two CPU readings, and that the oracle alone may judge the device on them
    (tests/test_gpu_sphere_scenes.py);
  * the launch's axis pairs, as the host probe reports what rmd::derive_scene_objects made of the scene, equal sphere_scenes.expected_axis_pairs —
    a reading of the rule, field by field — and are what the class names: all three fields for shuffled_room, none for tilted_pairs and irregular,
    the index-1022 pair and NOT the index-1023 / 1024 one for the thousand-object rooms of table_edges, ...; the candidate sets are on where the
    class intends them and off under the thin lens and in an irregular scene;
  * check_tiles of tests/test_primary_candidates.py on every case whose sets are on: a dropped object is never the oracle's hit and the closest
    hit over the candidates is the oracle's, bit for bit.
"""
import math

import numpy as np
import pytest

import sphere_scenes as ss
from raymond_amd import probe
from raymond_amd.scene import Plane, Sphere
from test_primary_candidates import check_tiles, wave_tiles
from test_second_reading import hold_oracle_to_second_reading

CASES = ss.cases()
IDS = [ss.case_id(c) for c in CASES]


def fields_of(launch_pairs):
    return [(launch_pairs >> (10 * k)) & 1023 for k in range(3)]


def test_every_class_has_two_seeds_and_the_lens_classes_their_variants():
    assert set(ss.SEEDS) == set(ss.CLASSES) and all(len(s) >= 2 for s in ss.SEEDS.values())
    for name in ss.LENS_CLASSES:
        assert sum(1 for c in CASES if c[0] == name and c[2]) >= 2
    for case in CASES:  # seeded and deterministic: the same objects twice
        a, b = ss.build(case), ss.build(case)
        assert [(type(o.geometry), o.geometry.origin, o.material.kind, o.material.color, o.material.roughness) for o in a[0].objects] == [
            (type(o.geometry), o.geometry.origin, o.material.kind, o.material.color, o.material.roughness) for o in b[0].objects]
        assert a[1].transform.position == b[1].transform.position and a[2].seed == b[2].seed
        spp = ss.THOUSAND_SPP if len(a[0].objects) > 1000 else ss.SPP
        assert a[2].sample_count == spp >= 128 and a[2].bounce_limit in ss.BOUNCE_LIMITS and a[2].use_dof == case[2]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_oracle_equals_the_second_reading_on_the_class(oracle, case):
    scene, cam, st, note = ss.build(case)
    W, H = cam.backbuffer_width, cam.backbuffer_height
    rng = np.random.default_rng([0x5EC0, case[1], int(case[2])] + [ord(c) for c in case[0]])
    thousand = len(scene.objects) > 1000  # (the pure-Python reading visits every object at every vertex)
    n_px, per_px = (6, 2) if thousand else (16, 3)
    pixels = sorted({(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(n_px)})
    # an object many of these paths meet, for hold_oracle_to_second_reading's "the paths go somewhere" clause: the commonest first vertex
    osc = oracle.OracleScene(scene)
    firsts = [int(osc.trace_sample_path(cam, st, x, y, s)[1][0]) for (x, y) in pixels for s in range(per_px)]
    want = max(set(firsts), key=firsts.count)
    black = case[0] == "one_lobe" and case[1] % 4 in (1, 2)  # every object black Diffuse, or Metal with nothing that emits: no radiance, by construction
    depths = hold_oracle_to_second_reading(oracle, scene, st, pixels, per_px, want_depths=(), want_object=want, min_nonzero=-1 if black else 0,
                                           vertices_every=1)
    print("%s: %d samples, vertices per path %s (%s)" % (ss.case_id(case), len(firsts), dict(sorted(depths.items())), note))
    assert sum(depths.values()) == len(pixels) * per_px


def containing_spheres(scene, cam):
    return [i for i, o in enumerate(scene.objects)
            if isinstance(o.geometry, Sphere) and math.dist(o.geometry.origin, cam.transform.position) < o.geometry.radius]


def unseen_spheres(scene, cam):
    """spheres whose centre makes 90 degrees or more with EVERY direction of the frame (with its four corner directions (px, py, 1): the frame's
    directions are their convex cone): behind the camera for every tile, so no tile's cone has phi + theta < 90 degrees and the bit stays"""
    ey = math.tan(math.radians(cam.fov_vert) / 2.0)
    ex = ey * cam.backbuffer_width / cam.backbuffer_height
    out = []
    for i, o in enumerate(scene.objects):
        if isinstance(o.geometry, Sphere):
            v = [a - b for a, b in zip(o.geometry.origin, cam.transform.position)]
            if all(v[0] * sx * ex + v[1] * sy * ey + v[2] <= 0.0 for sx in (-1.0, 1.0) for sy in (-1.0, 1.0)):
                out.append(i)
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_class_exercises_what_it_names(oracle, product_lib, case):
    name, seed, lens = case
    scene, cam, st, note = ss.build(case)
    tiles = wave_tiles(cam.backbuffer_width, cam.backbuffer_height)
    stats = dict(tiles=0, rays=0, spheres_dropped=0, pairs_dropped=0)
    rng = np.random.default_rng(seed)
    launch_visit, launch_pairs, on, visit, pairs = probe.primary_candidates(cam, st, scene, tiles)
    fields, n = fields_of(launch_pairs), len(scene.objects)
    print("%s: %d objects, axis pairs %s, candidate sets %s (%s)" % (ss.case_id(case), n, fields, "on" if on else "off", note))
    # the table, by the rule
    assert launch_pairs < 1 << 30 and fields == ss.expected_axis_pairs(scene)
    planes = [i for i, o in enumerate(scene.objects) if isinstance(o.geometry, Plane)]
    for k, f in enumerate(fields):
        if f:  # the field names the later plane of a pair of walls +-e_k, and the launch's turns pass it by
            later = scene.objects[f - 1].geometry
            assert isinstance(later, Plane) and abs(later.normal[k]) == 1.0 and sum(c != 0.0 for c in later.normal) == 1
            assert f - 1 >= 64 or not (launch_visit >> (f - 1)) & 1
    for i in range(min(n, 64)):  # every object that is no plane has a turn
        if i not in planes:
            assert (launch_visit >> i) & 1
    # the candidate sets: on where the class intends them
    assert on == (not lens and name != "irregular")
    if name in ("shuffled_room", "signed_zero_normals", "camera_on_walls", "coincident_spheres", "one_lobe", "rough_extremes", "fov_and_aspect", "duplicate_walls"):
        assert all(fields)
    if name in ("tilted_pairs", "irregular"):
        assert not any(fields)
    if name == "partial_room":
        assert 1 <= sum(f != 0 for f in fields) <= 2 and len(planes) > 2 * sum(f != 0 for f in fields)
    if name == "duplicate_walls":
        assert len(planes) == 11  # three pairs for the axis rule, and five planes it leaves to the general tests
    if name == "table_edges":
        kind, n_spheres = ss.TABLE_EDGES[seed % len(ss.TABLE_EDGES)]
        later = sorted((n_spheres + 1, n_spheres + 3, n_spheres + 5))
        want = sorted(j + 1 if j <= 1022 else 0 for j in later)  # index 1022 is the field's last value, 1023 its first overflow
        assert sorted(fields) == want, (fields, want)
        if kind == "thousand":
            assert (1023 in fields) == (1022 in later) and sum(f == 0 for f in fields) == sum(j > 1022 for j in later)
        else:
            assert min(planes) == n_spheres and all(fields)
    if not on:
        assert (visit == np.uint64(launch_visit)).all() and (pairs == np.uint32(launch_pairs)).all()
        return
    on2, *_ = check_tiles(oracle, scene, cam, st, tiles, rng, stats)
    assert on2
    print("  ", stats)
    inside = ss.camera_strictly_inside(scene, cam)
    if name == "camera_on_walls":
        where = ss.CAMERA_ON_WALLS[seed % len(ss.CAMERA_ON_WALLS)][2]
        assert (False in inside) == (where != "inside")
        if where != "inside":  # on a wall's coordinate or outside it: no pair is dropped on any tile
            assert stats["pairs_dropped"] == 0 and (pairs == np.uint32(launch_pairs)).all()
        else:  # one step inside: the wall an ulp away is every facing ray's nearest, and that pair may legitimately stay alone (check_tiles held it)
            assert stats["pairs_dropped"] > 0
    elif name in ("shuffled_room", "signed_zero_normals", "duplicate_walls", "coincident_spheres", "one_lobe", "rough_extremes", "fov_and_aspect", "table_edges"):
        assert False not in inside and stats["pairs_dropped"] > 0  # walls in either order, and the sets still find the pair to keep
    if name == "coincident_spheres":
        kept = containing_spheres(scene, cam) + unseen_spheres(scene, cam)
        assert len(containing_spheres(scene, cam)) == 2 and len(unseen_spheres(scene, cam)) == 1 and len(set(kept)) == 3
        for i in kept:  # a sphere that contains the camera, and one behind it, keeps its bit on every tile
            assert all((int(v) >> i) & 1 for v in visit), i
        assert stats["spheres_dropped"] > 0
    if name == "fov_and_aspect":  # TileCone.ok true and false within one frame: some tiles drop, and at the wide angle some cannot
        dropping = np.array([int(v) != launch_visit or int(p) != launch_pairs for v, p in zip(visit, pairs)])
        assert dropping.any()
        if cam.fov_vert > 90.0:
            assert not dropping.all()
