"""The adversarial scenes of tests/mesh_scenes.py on the CPU: are they a fair yardstick, and is each class what it says?

For every class and seed (and the thin-lens variants):
  * the oracle equals the second reading of the source (tests/second_reading.py) on a seeded list of (x, y, sample) triples — N_PIXELS pixels, half
    of them drawn among the pixels whose primary ray enters a grid's box where there are such, SAMPLES_PER_PIXEL samples each: 288 triples a case,
    17,280 in all, which keeps this file well under a minute — at the bar of test_second_reading.py's mesh case and more: the radiance bit for bit (NaN
    for NaN) and EVERY vertex sequence the same.  The scenes are built on exact ties — one AccGrid in two objects, two grids of one mesh, a camera
    ON a wall or ON a face of the box — so this is what shows that they do not split the two CPU readings, and that the oracle alone may judge the
    device on them (tests/test_gpu_mesh_scenes.py).  No class uses a mesh of grid_meshes.SLOW_IN_PYTHON;
  * the class is what it names, from data available without a device: the host probe's launch fields (rmd_probe_primary_candidates: visit mask,
    axis pairs) against sphere_scenes.expected_axis_pairs, the grids' own tables (resolution, run lengths), plain geometry (which primary rays
    enter which box) and the oracle's vertex sequences.  What only the library knows (n_grid_objects, mask_shift, walk_steps_bound) the GPU test
    asserts through rmd_probe_scene_plan.
"""
import numpy as np
import pytest

import grid_meshes as gm
import mesh_scenes as ms
import sphere_scenes as ss
from raymond_amd import abi, probe
from raymond_amd.scene import Grid, Object, Plane, Scene, Sphere
from test_primary_candidates import wave_tiles
from test_second_reading import hold_oracle_to_second_reading

CASES = ms.cases()
IDS = [ms.case_id(c) for c in CASES]
N_PIXELS, SAMPLES_PER_PIXEL = 48, 6
BLACK = ()  # no case is black by construction: every scene holds something that emits, in reach of the camera's paths


def fields_of(launch_pairs):
    return [(launch_pairs >> (10 * k)) & 1023 for k in range(3)]


def entering(scene, cam):
    """per pixel (row-major): does its primary ray through the pixel centre enter the box of any grid"""
    d = ms.primary_directions(cam)
    out = np.zeros(d.shape[0], dtype=bool)
    for g in ms.distinct_grids(scene):
        out |= ms.rays_entering(g, cam.transform.position, d)
    return out


def pixels_of(case, scene, cam):
    W, H = cam.backbuffer_width, cam.backbuffer_height
    rng = np.random.default_rng([0x3E5C, case[1], int(case[2])] + [ord(c) for c in case[0]])
    inside = np.flatnonzero(entering(scene, cam))
    picked = set()
    if len(inside):
        picked |= {int(i) for i in rng.choice(inside, size=min(N_PIXELS // 2, len(inside)), replace=False)}
    while len(picked) < N_PIXELS:
        picked.add(int(rng.integers(0, W * H)))
    return sorted((i % W, i // W) for i in picked)


def without_grids(scene):
    """the scene with a unit sphere in every grid object's place: what sphere_scenes' reading of the axis-pair rule needs (indices kept)"""
    plain = Scene()
    plain.objects = [Object(Sphere((0.0, 0.0, 0.0), 1.0), o.material) if isinstance(o.geometry, Grid) else o for o in scene.objects]
    return plain


def test_every_class_has_two_seeds_and_the_lens_classes_their_variants():
    assert set(ms.SEEDS) == set(ms.CLASSES) and all(len(s) >= 2 for s in ms.SEEDS.values())
    assert {"shared_grid", "camera_in_box", "every_ray_walks", "mirror_box"} <= set(ms.LENS_CLASSES) and ms.APERTURE == ss.APERTURE
    for name in ms.LENS_CLASSES:
        assert sum(1 for c in CASES if c[0] == name and c[2]) >= 2
    W, H = ms.FRAME
    assert W % 8 and H % 8 and 900 <= W * H <= 1300 and ms.SPP == 48  # ragged wave tiles on both edges, about a thousand pixels
    limits = set()
    for case in CASES:  # seeded and deterministic: the same objects and the same grids twice
        a, b = ms.build(case), ms.CLASSES[case[0]](case[1], lens=case[2])
        assert len(a[0].objects) == len(b[0].objects)
        for oa, ob in zip(a[0].objects, b[0].objects):
            assert type(oa.geometry) is type(ob.geometry) and (oa.material.kind, oa.material.color, oa.material.roughness) == (ob.material.kind, ob.material.color, ob.material.roughness)
            if isinstance(oa.geometry, Grid):
                ga, gb = oa.geometry.grid, ob.geometry.grid
                assert ga.tri_pos.tobytes() == gb.tri_pos.tobytes() and ga.cells.tobytes() == gb.cells.tobytes() and ga.mapping_table.tobytes() == gb.mapping_table.tobytes()
            else:
                assert oa.geometry.origin == ob.geometry.origin
        assert a[1].transform.position == b[1].transform.position and a[2].seed == b[2]["seed"]
        st = a[2]
        assert st.sample_count == ms.SPP and st.tile_size == (32, 32) and st.bounce_limit in ms.BOUNCE_LIMITS and st.use_dof == case[2]
        assert (a[1].backbuffer_width, a[1].backbuffer_height) == ms.FRAME and (a[1].aperture_radius == ms.APERTURE) == case[2]
        assert ms.grid_objects(a[0]), case
        for g in ms.distinct_grids(a[0]):  # the device's builder is not involved, but its bound on a run holds for whoever uploads these
            assert gm.runs(g).max() <= gm.MAX_RUN
        limits.add(st.bounce_limit)
    assert limits == set(ms.BOUNCE_LIMITS)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_oracle_equals_the_second_reading_on_the_class(oracle, case):
    scene, cam, st, note = ms.build(case)
    pixels = pixels_of(case, scene, cam)
    osc = oracle.OracleScene(scene)
    firsts = [int(osc.trace_sample_path(cam, st, x, y, s)[1][0]) for (x, y) in pixels for s in range(SAMPLES_PER_PIXEL)]
    hits = [v for v in firsts if v >= 0]  # (-1: the primary ray misses everything)
    want = max(set(hits), key=hits.count)  # an object many of these paths meet, for the "paths go somewhere" clause
    depths = hold_oracle_to_second_reading(oracle, scene, st, pixels, SAMPLES_PER_PIXEL, want_depths=(), want_object=want,
                                           min_nonzero=-1 if ms.case_id(case) in BLACK else 0, vertices_every=1)
    print("%s: %d samples, vertices per path %s (%s)" % (ms.case_id(case), len(firsts), dict(sorted(depths.items())), note))
    assert sum(depths.values()) == len(pixels) * SAMPLES_PER_PIXEL == N_PIXELS * SAMPLES_PER_PIXEL


def sampled_paths(oracle, scene, cam, st, n_pixels=48, per_px=2, seed=5):
    """the oracle's vertex sequences (object index per vertex, -1 = a miss) on a seeded list of pixels"""
    rng = np.random.default_rng(seed)
    osc = oracle.OracleScene(scene)
    W, H = cam.backbuffer_width, cam.backbuffer_height
    out = []
    for _ in range(n_pixels):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        out += [osc.trace_sample_path(cam, st, x, y, s)[1].tolist() for s in range(per_px)]
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_class_is_what_it_says(oracle, product_lib, case):
    name, seed, lens = case
    scene, cam, st, note = ms.build(case)
    objs, n = scene.objects, len(scene.objects)
    grids_at, grids = ms.grid_objects(scene), ms.distinct_grids(scene)
    planes = [i for i, o in enumerate(objs) if isinstance(o.geometry, Plane)]
    launch_visit, launch_pairs, on, _, _ = probe.primary_candidates(cam, st, scene, wave_tiles(cam.backbuffer_width, cam.backbuffer_height)[:1])
    fields = fields_of(launch_pairs)
    enter = entering(scene, cam)
    pos = cam.transform.position
    print("%s: %d objects, grids at %s, axis pairs %s, %d of %d primary rays enter a box (%s)" % (ms.case_id(case), n, grids_at, fields, enter.sum(), enter.size, note))
    # the launch, by the rule: the axis pairs of the scene's planes whatever the grids; no candidate sets in a scene with a grid; every grid has a turn
    assert not on and launch_pairs < 1 << 30 and fields == ss.expected_axis_pairs(without_grids(scene))
    for i in range(min(n, 64)):
        if i not in planes:
            assert (launch_visit >> i) & 1, i
    for k, f in enumerate(fields):
        if f:
            later = objs[f - 1].geometry
            assert isinstance(later, Plane) and abs(later.normal[k]) == 1.0 and (f - 1 >= 64 or not (launch_visit >> (f - 1)) & 1)
    paths = sampled_paths(oracle, scene, cam, st, n_pixels=200 if name == "no_ray_enters" else 48) if name in ("shared_grid", "camera_in_box", "every_ray_walks", "mirror_box", "no_ray_enters", "grid_positions") else []
    through_grid = sum(any(v in grids_at for v in p) for p in paths)

    if name == "shared_grid":
        assert len(grids_at) == 2 and len(grids) == (1 if seed < 2 else 2)
        a, b = objs[grids_at[0]], objs[grids_at[1]]
        ga, gb = a.geometry.grid, b.geometry.grid
        assert (ga is gb) == (seed < 2) and ga.tri_pos.tobytes() == gb.tri_pos.tobytes() and ga.tri_nrm.tobytes() == gb.tri_nrm.tobytes()
        assert ga.cells.tobytes() == gb.cells.tobytes() and ga.mapping_table.tobytes() == gb.mapping_table.tobytes() and ga.bbox_min.tobytes() == gb.bbox_min.tobytes()
        assert (a.material.kind, a.material.color) != (b.material.kind, b.material.color)
        # every grid hit is an exact tie: the lower index wins it, always
        assert through_grid > 10 and not any(grids_at[1] in p for p in paths)
    if name == "grid_positions":
        where = ms.GRID_POSITIONS[seed % len(ms.GRID_POSITIONS)]
        assert grids_at == [n - 1 if k == "last" else k for k in where] and len(planes) == 6 and all(fields) and through_grid > 5
        if seed % len(ms.GRID_POSITIONS) == 5:
            assert grids_at[0] < 64 < grids_at[1]
        if max(grids_at) >= 64:  # the fillers past the mask's reach are hit as well: next_turn counts on
            assert n > 64
    if name == "three_grids":
        assert len(grids_at) == 3 and len(grids) == 3 and all(fields)
        if seed >= 2:  # 256 bytes of mask budget over three grids: 21 words each, fewer than one bit per cell needs
            assert ms.scene_tunables(case) == {abi.RMD_TUNE_MASK_BUDGET: 256}
            covered = [int(np.flatnonzero(gm.runs(g))[-1]) + 1 for g in grids]  # (a mask covers the cells up to the last non-empty one)
            assert all((c + 31) // 32 + 1 > 256 // 4 // 3 for c in covered), covered
        else:
            assert ms.scene_tunables(case) == {}
    if name == "camera_in_box":
        g = grids[0]
        which = seed % 4
        inside = [g.bbox_min[k] < pos[k] < g.bbox_max[k] for k in range(3)]
        if which in (0, 1):
            assert all(inside) and enter.all()
        if which == 1:  # a closed mesh around the camera: every path's first vertex is the mesh or the light inside it
            light = [i for i, o in enumerate(objs) if isinstance(o.geometry, Sphere)]
            assert all(p[0] in grids_at + light for p in paths) and through_grid > len(paths) // 2
        if which == 2:
            assert pos[2] == g.bbox_min[2] and inside[:2] == [True, True] and enter.all()
        if which == 3:
            assert pos[0] == g.bbox_max[0] and inside[1:] == [True, False] and 0 < enter.sum() < enter.size
    if name == "camera_on_wall_with_mesh":
        assert False in ss.camera_strictly_inside(without_grids(scene), cam) and all(fields) and len(grids_at) == 1
        assert any(isinstance(o.geometry, Plane) and sum((p - q) * c for p, q, c in zip(pos, o.geometry.origin, o.geometry.normal)) == 0.0 for o in objs)
        assert enter.sum() > 20
    if name == "no_ray_enters":
        assert not enter.any()
        if seed < 2:
            assert not planes and all(o.material.kind == abi.RMD_MAT_EMISSION for i, o in enumerate(objs) if i not in grids_at) and through_grid == 0
        else:
            assert len(planes) == 6 and through_grid > 0 and not any(p[0] in grids_at for p in paths)  # only bounce rays reach the mesh
    if name == "every_ray_walks":
        first_is_grid = sum(p[0] in grids_at for p in paths)
        assert enter.all() and ((first_is_grid < len(paths) // 4) if seed < 2 else (first_is_grid > len(paths) * 3 // 4)), (first_is_grid, len(paths))
    if name == "mirror_box":
        m = objs[grids_at[0]].material
        g = grids[0]
        assert st.bounce_limit == 16 and m.kind == abi.RMD_MAT_METAL and 0.0 < m.roughness <= 0.03 and all(g.bbox_min[k] < pos[k] < g.bbox_max[k] for k in range(3))
        assert sum(len(p) == 16 and p[-1] >= 0 for p in paths) > len(paths) // 4, "paths live to the limit"
    if name in ("one_cell", "few_cells"):
        res, runs = [int(v) for v in grids[0].resolution], gm.runs(grids[0])
        mesh_name = (ms.ONE_CELL if name == "one_cell" else ms.FEW_CELLS)[seed]
        if name == "one_cell":
            assert res == [[1, 1, 1], [2, 1, 1], [3, 1, 1]][seed] and sum(res) + 3 <= 8 and (seed or sum(res) + 3 == 6)
        elif mesh_name in ("cluster", "spanning"):
            assert runs.max() >= 512  # hundreds in one cell: many full chunks in one walk
        else:
            assert int(np.prod(res)) in (8, 27)
        assert enter.sum() > 100
    if name == "thin_and_flat":
        g = grids[0]
        axis = 2 if seed % 2 == 0 else 0
        assert int(g.resolution[axis]) == 1 and g.bbox_max[axis] - g.bbox_min[axis] == ms.FLAT and min(int(v) for v in g.resolution) == 1
        assert enter.sum() > (100 if axis == 2 else 0)
    if name == "materials":
        m = objs[grids_at[0]].material
        assert (m.kind, m.color == (0.0, 0.0, 0.0), m.roughness == 0.0 and m.kind == abi.RMD_MAT_METAL) == (
            (abi.RMD_MAT_EMISSION, False, False), (abi.RMD_MAT_DIFFUSE, True, False), (abi.RMD_MAT_METAL, False, True))[seed % 3]
        assert ss.is_regular(without_grids(scene)) == (seed % 3 != 2) and len(ms.render_flags(case)) == 2
    if name == "nan_normals":
        g = grids[0]
        assert np.isnan(g.tri_pos).sum() == 1 if seed % 2 == 0 else (np.isnan(g.tri_nrm).any(axis=1).sum() >= 10 and not np.isnan(g.tri_pos).any())
    if name == "open_scene":
        assert not planes and launch_pairs == 0 and enter.sum() > 100
    if name == "partial_room_with_mesh":
        later = [f - 1 for f in fields if f]
        assert 1 <= len(later) <= 2 and len(planes) > 2 * len(later) and grids_at == ([0] if seed % 2 == 0 else [n - 1])
        assert all(j > grids_at[0] for j in later) if seed % 2 == 0 else all(j < grids_at[0] for j in later)
