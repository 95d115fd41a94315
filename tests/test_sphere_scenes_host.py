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
    hit over the candidates is the oracle's, bit for bit;
  * the classes aimed at the tile classes (ss.TILE_CLASS_CLASSES) hold, by the host probe rmd_probe_tile_classes, the tiles they were built to
    hold — at least a third of the wave tiles classed in every non-lens case of one_wall_mixed, emitter_colours, black_walls and ragged_one_wall,
    at least 60 BLACK and 60 EMITTER tiles together, all three kinds in one_wall_mixed with BLACK tiles at bounce limits 1 and 2, the seed's
    colour on emitter_colours' wall, the black Metal wall's tiles general, classed tiles at 63 and 64 objects and none at 65, classed tiles one
    pixel wide and high, classes off under the lens, both classes under both rect lists of the GPU test — and every classed tile passes
    test_tile_classes.check_classed_tile against the oracle, at every one of its pixels;
  * the frames discriminate: the tile rule read from the oracle's side, with either of two mistakes the kernel's rule could make (a tile classed
    at 65 objects by the visit mask alone; a black Metal wall taken for BLACK), leaves the oracle's samples on a named new case — the stand-in
    for a wrong kernel, which is never run on a device.
"""
import math

import numpy as np
import pytest

import sphere_scenes as ss
from raymond_amd import abi, probe
from raymond_amd.scene import Plane, Sphere
from test_primary_candidates import check_tiles, tile_rays, wave_tiles
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


def rect_wave_tiles(rects, W, H):
    """the 8x8 wave tiles the library cuts from a rect list: from each rect's own origin (tests/test_gpu_tile_classes.py)"""
    return np.array([(x, y, min(8, min(tx + tw, W) - x), min(8, min(ty + th, H) - y)) for tx, ty, tw, th in rects
                     for y in range(ty, min(ty + th, H), 8) for x in range(tx, min(tx + tw, W), 8)], dtype=np.uint32)


def class_counts(case):
    """-> (on, emitter tiles, black tiles, wave tiles) of a case, by the host probe"""
    scene, cam, st, _ = ss.build(case)
    on, cls, _ = probe.tile_classes(cam, st, scene, wave_tiles(cam.backbuffer_width, cam.backbuffer_height))
    return on, int((cls == probe.TILE_EMITTER).sum()), int((cls == probe.TILE_BLACK).sum()), len(cls)


def the_tile_classes_are_what_the_class_names(oracle, case, scene, cam, st, tiles, rng):
    """One case of the classes aimed at the tile classes (ss.TILE_CLASS_CLASSES): the probe's classes are the ones the class was built to have, and
    every classed tile holds against the oracle (test_tile_classes.check_classed_tile: the rays hit the predicted wall, an EMITTER sample is the
    colour bit for bit, a BLACK sample with low lobe bits is zero)."""
    from test_tile_classes import check_classed_tile

    name, seed, lens = case
    W, H = cam.backbuffer_width, cam.backbuffer_height
    on, cls, wall = probe.tile_classes(cam, st, scene, tiles)
    emitter, black, general = cls == probe.TILE_EMITTER, cls == probe.TILE_BLACK, cls == probe.TILE_GENERAL
    print("   tile classes %s: %d EMITTER, %d BLACK, %d general of %d wave tiles, bounce limit %d" % (
        "on" if on else "off", emitter.sum(), black.sum(), general.sum(), len(tiles), st.bounce_limit))
    if lens:
        assert not on and general.all() and (wall == -1).all()
        return
    assert on
    if name != "class_table_edge":
        assert 3 * int((~general).sum()) >= len(tiles), "fewer than a third of the wave tiles are classed"
    if name == "one_wall_mixed":
        assert black.any() and emitter.any() and general.any()  # (every seed holds all three; the issue asks it of two)
        assert st.bounce_limit == ss.BOUNCE_LIMITS[seed % 4]
        from test_gpu_sphere_scenes import rect_lists

        for rects in rect_lists(W, H):  # the off-lattice rect lists of the GPU test reach both classes too
            _, rc, _ = probe.tile_classes(cam, st, scene, rect_wave_tiles(rects, W, H))
            assert (rc == probe.TILE_BLACK).any() and (rc == probe.TILE_EMITTER).any(), rects[:2]
    if name == "emitter_colours":
        assert emitter.all() and len(set(wall)) == 1
        got, want = np.array(scene.objects[int(wall[0])].material.color), np.array(ss.EMITTER_COLOURS[seed])
        assert got.tobytes() == want.tobytes()  # the seed's colour, signs of zero and denormals as written
    if name == "black_walls":
        assert black.any() and not emitter.any()
        metal = ss.black_metal_wall(scene)
        assert (metal is not None) == (seed == 3)
        if metal is None:
            assert black.all() or (ss.BLACK_WALLS[seed][2] == 1e-12 and black.sum() == len(tiles) - 1)  # (one tile holds the small light)
        else:  # the black Metal wall is what most of the general tiles see (the oracle's hits at the tile centres), and none of them is classed
            assert general.any() and metal not in set(wall)
            centres = np.array([(t[0] + t[2] // 2, t[1] + t[3] // 2) for t in tiles], dtype=np.uint32)
            rays, ok = oracle.sample_primary_rays(cam, st.seed, False, centres, np.zeros(len(tiles), dtype=np.uint32))
            hit = oracle.OracleScene(scene).scene_intersect(rays)[0]
            assert ok.all() and (hit[general] == metal).sum() >= 3 and not (hit[~general] == metal).any()
        back = scene.objects[int(wall[black][0])].material
        assert back.roughness == ss.BLACK_WALLS[seed][2] and np.array(back.color).tobytes() == np.array(ss.BLACK_WALLS[seed][1]).tobytes()
        assert {"first": int(wall[black][0]) == 0, "last": int(wall[black][0]) == len(scene.objects) - 1}.get(ss.BLACK_WALLS[seed][3], True)
    if name == "class_table_edge":
        assert len(scene.objects) == ss.CLASS_TABLE_EDGE[seed]
        if len(scene.objects) <= 64:
            assert black.sum() >= 3 and emitter.any() and general.any()
        else:
            assert general.all()
    if name == "ragged_one_wall":
        assert (W, H) == ss.RAGGED_ONE_WALL[seed][0]
    full = oracle.OracleScene(scene)
    stats = dict(rays=0, emitter_samples=0, black_zero_samples=0, black_survivors=0)
    for tile, c, w in zip(tiles, cls, wall):
        if c != probe.TILE_GENERAL:
            check_classed_tile(oracle, full, scene, cam, st, tile, int(c), int(w), rng, stats, every_pixel=True)
    print("  ", stats)


def test_the_new_classes_together_reach_the_tile_classes(product_lib):
    """What no single case can show: the counts over the classes, the kinds per seed, the ragged tiles."""
    total, mixed_seeds, black_at = dict(emitter=0, black=0), 0, set()
    thin = dict(w=0, h=0, black=0)
    for case in ss.cases(ss.TILE_CLASS_CLASSES, lens=False):
        scene, cam, st, _ = ss.build(case)
        tiles = wave_tiles(cam.backbuffer_width, cam.backbuffer_height)
        on, cls, _ = probe.tile_classes(cam, st, scene, tiles)
        e, b = int((cls == probe.TILE_EMITTER).sum()), int((cls == probe.TILE_BLACK).sum())
        print("%-22s %3d EMITTER %3d BLACK of %3d wave tiles, bounce limit %2d" % (ss.case_id(case), e, b, len(tiles), st.bounce_limit))
        total["emitter"] += e
        total["black"] += b
        if case[0] == "one_wall_mixed":
            mixed_seeds += bool(e and b and e + b < len(tiles))
            if b:
                black_at.add(st.bounce_limit)
        if case[0] == "ragged_one_wall":
            classed = cls != probe.TILE_GENERAL
            thin["w"] += int((classed & (tiles[:, 2] == 1)).sum())
            thin["h"] += int((classed & (tiles[:, 3] == 1)).sum())
            thin["black"] += int(((cls == probe.TILE_BLACK) & ((tiles[:, 2] == 1) | (tiles[:, 3] == 1))).sum())
    print(total, thin)
    assert total["black"] >= 60 and total["emitter"] >= 60, total
    assert mixed_seeds >= 2 and {1, 2} <= black_at, (mixed_seeds, black_at)
    assert thin["w"] >= 1 and thin["h"] >= 1 and thin["black"] >= 1, thin
    frames = {ss.build(c)[1].backbuffer_width * 1000 + ss.build(c)[1].backbuffer_height for c in ss.cases(("ragged_one_wall",))}
    assert {1001, 1008, 9009, 41025, 7033, 33007} <= frames
    n63, n64, n65 = (class_counts(("class_table_edge", s, False)) for s in (0, 1, 2))
    assert n63[1] + n63[2] > 0 and n64[1] + n64[2] > 0 and n65[1] + n65[2] == 0 and n65[0]  # (the classes are ON at 65 objects: it is the tile rule that refuses)


# ---------------------------------------------------------------- the frames discriminate: two wrong readings of the tile rule
# No wrong kernel is run on a device.  Its stand-in: the tile rule read from the oracle's side — a tile is classed when every ray the oracle makes
# for it (test_primary_candidates.tile_rays) hits one and the same wall of the table and that wall emits or is black Diffuse — with two mistakes
# the kernel's rule could make.  Each must leave the oracle's answer on a named new case; without a mistake the reading never does.
MISTAKES = {"mask_alone_at_65": "class_table_edge-2",  # looks at the 64 objects a visit mask reaches and not at the table's length
            "black_metal_is_black": "black_walls-3"}  # takes colour == 0 for the BLACK class whatever prob_d is


def misread_frame(oracle, case, mistake=None):
    """-> (tiles classed, samples that are not what the class says) over every pixel of every tile the reading classes, four samples each"""
    scene, cam, st, _ = ss.build(case)
    tiles = wave_tiles(cam.backbuffer_width, cam.backbuffer_height)
    rng = np.random.default_rng(7)
    objects = scene.objects[:64] if mistake == "mask_alone_at_65" else scene.objects
    if mistake is None and len(scene.objects) > 64:
        return 0, 0
    seen, full = oracle.OracleScene(ss._scene_of(objects)), oracle.OracleScene(scene)
    classed = off = 0
    for tile in tiles:
        hit = np.unique(seen.scene_intersect(tile_rays(oracle, cam, tile, rng))[0])
        if len(hit) != 1 or hit[0] < 0 or not isinstance(objects[int(hit[0])].geometry, Plane):
            continue
        m = objects[int(hit[0])].material
        black = tuple(m.color) == (0.0, 0.0, 0.0) and (m.kind == abi.RMD_MAT_DIFFUSE or (mistake == "black_metal_is_black" and m.kind == abi.RMD_MAT_METAL))
        if m.kind != abi.RMD_MAT_EMISSION and not black:
            continue
        classed += 1
        x0, y0, w, h = (int(v) for v in tile)
        xy = np.array([(x, y) for y in range(y0, y0 + h) for x in range(x0, x0 + w) for _ in range(4)], dtype=np.uint32)
        smp = np.tile(np.arange(4, dtype=np.uint32), w * h)
        rgb = full.trace_samples(cam, st, xy, smp)
        if m.kind == abi.RMD_MAT_EMISSION:
            off += int((rgb.view(np.uint64) != np.array(m.color).view(np.uint64)[None, :]).any(axis=1).sum())
        else:
            r22 = oracle.block_uniforms(st.seed, xy[:, 1].astype(np.int64) * cam.backbuffer_width + xy[:, 0], smp, np.zeros(len(smp), dtype=np.int64))[:, 2]
            off += int((rgb[r22 * 4194304.0 < float(1 << 21)] != 0.0).any(axis=1).sum())
    return classed, off


@pytest.mark.parametrize("name", ["one_wall_mixed-1", "black_walls-3", "class_table_edge-1", "class_table_edge-2", "ragged_one_wall-2"])
def test_the_reading_without_a_mistake_never_leaves_the_oracle(oracle, product_lib, name):
    case = next(c for c in CASES if ss.case_id(c) == name)
    classed, off = misread_frame(oracle, case)
    print("%s: %d tiles classed by the reading, %d samples off" % (name, classed, off))
    assert off == 0 and (classed > 0) == (name != "class_table_edge-2")
    assert classed >= sum(class_counts(case)[1:3])  # (the reading samples rays; the kernel's rule proves: it classes no more than this)


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_each_mistake_leaves_the_oracle_on_a_named_new_case(oracle, product_lib, mistake):
    case = next(c for c in CASES if ss.case_id(c) == MISTAKES[mistake])
    right, wrong = misread_frame(oracle, case), misread_frame(oracle, case, mistake)
    print("%s on %s: %d tiles classed (%d without the mistake), %d samples are not what the class says" % (mistake, MISTAKES[mistake], wrong[0], right[0], wrong[1]))
    assert wrong[0] > right[0] and wrong[1] > 0 and right[1] == 0, "the mistake %s stays on the oracle's answer on %s" % (mistake, MISTAKES[mistake])


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
    if name in ("shuffled_room", "signed_zero_normals", "camera_on_walls", "coincident_spheres", "one_lobe", "rough_extremes", "fov_and_aspect", "duplicate_walls") + ss.TILE_CLASS_CLASSES:
        assert all(fields)
    if name in ss.TILE_CLASS_CLASSES:
        the_tile_classes_are_what_the_class_names(oracle, case, scene, cam, st, tiles, rng)
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
    elif name in ("shuffled_room", "signed_zero_normals", "duplicate_walls", "coincident_spheres", "one_lobe", "rough_extremes", "fov_and_aspect", "table_edges") + ss.TILE_CLASS_CLASSES:
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
