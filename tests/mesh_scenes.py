"""Adversarial scenes for the render kernel of scenes WITH grids (render_kernel.hpp: render_wave_queued / render_wave<.., CHAIN>, scene_split.hpp:
intersect_simple / intersect_grids, their planning in api.cpp) — plain numpy, no GPU, no oracle.

Every form-against-form test of the mesh kernel used to render one of two worlds (one lumpy sphere in the six-wall room; two lumpy spheres between
four planes), with the stock camera strictly inside the room.  What the kernel decides once per scene or per launch — walk_cut (on only with ONE
grid object), visit_mask / grid_mask and next_turn's walk over them, the axis pairs handled ahead of the object loops, axis_pair_test's
zero-numerator ballot, mask_shift from the mask budget divided by n_grids, walk_steps_bound in the queued form's trip bound, the lexicographic
merge of a grid hit with another hit of EQUAL distance, the packed queue words at bounce limit 16, the ratio of rays held to rays pushed — was seen
in one state.  The classes below put each of those into its other states.  tests/test_mesh_scenes_host.py holds the oracle to the second reading
of the source on every class and asserts that a class is what it says; tests/test_gpu_mesh_scenes.py then holds every launch form of the device to
form A byte for byte, and to the oracle.

The conventions and the API are tests/sphere_scenes.py's (whose room, dyadic coordinates and material makers are imported, not copied): one
function per class, seeded and deterministic, f(seed, lens=False) -> (Scene, CameraSettings, dict of Settings keywords, note); CLASSES, SEEDS (at
least two per class), LENS_CLASSES, cases(), case_id(), build().  Deliberate coincidences are EXACT: the same Python floats, the same arrays,
dyadic coordinates.  Grids are built with the host builder (AccGrid.build_from_mesh), never on the device; a class's scene is built once per
process (the tests read it, none changes it).  The camera has no rotation: it looks down +z.  A mesh's box is never deeper than tall (the
reference's res.z index quirk, Q5, wants size.z <= size.y of any mesh it can build a grid for).

What a class needs beyond the scene travels beside it: scene_tunables(case) names the tunables its DeviceScene is created under (three_grids'
mask budget) and render_flags(case) the rmd_settings flags it is rendered with besides 0 (materials).
"""
import functools
import math

import numpy as np

import grid_meshes as gm
import sphere_scenes as ss
from raymond_amd import abi, scenes
from raymond_amd.scene import AccGrid, CameraSettings, Grid, Material, Mesh, Object, Scene, Settings, Sphere, Transform
from sphere_scenes import APERTURE, BOUNCE_LIMITS, _black, _diffuse, _emission, _material, _metal, _room, _shuffled

SPP = 48
FRAME = (44, 27)  # 6 x 4 wave tiles, ragged on both edges: 1,188 pixels, 57,024 samples
MESH_SEED = 0x6D65  # grid_meshes.adversarial_meshes' seed here


# ---------------------------------------------------------------- parts
@functools.lru_cache(maxsize=None)
def _adversarial():
    return gm.adversarial_meshes(np.random.default_rng(MESH_SEED))


def _moved(mesh, t):
    m = Mesh(mesh.tri_pos.copy(), mesh.tri_nrm.copy())
    m.bake_transform(t)
    return m


def _grid(mesh):
    return Grid(AccGrid.build_from_mesh(mesh))


def _lumpy(n, extent, centre):
    return scenes.lumpy_sphere_mesh(n, extent=extent, centre=centre)


def _bounds(rng, lo_z=None):
    """sphere_scenes' room, its far wall and (for a mesh behind the camera) its near wall where a class wants them"""
    lo, hi = ss._bounds(rng)
    if lo_z is not None:
        lo[2] = lo_z
    return lo, hi


def _lit_room(rng, lo, hi, bounce_limit):
    """sphere_scenes' room; at bounce limit 1 only what the camera sees can light the frame, so the emitting wall is then the far one"""
    mats = ss._wall_materials(rng)
    if bounce_limit == 1:
        e = next(i for i, m in enumerate(mats) if m.kind == abi.RMD_MAT_EMISSION)
        mats[e], mats[5] = mats[5], mats[e]
    return _room(rng, lo, hi, mats)


def _camera(pos=(0.0, 0.0, 0.0), lens=False):
    return CameraSettings(FRAME[0], FRAME[1], 55.0, Transform(tuple(float(v) for v in pos)), focal_length=2.5, aperture_radius=APERTURE if lens else 0.0)


def _kw(seed, lens=False, bounce_limit=None, salt=0):
    b = BOUNCE_LIMITS[(seed + salt) % 4] if bounce_limit is None else bounce_limit
    return dict(sample_count=SPP, tile_size=(32, 32), bounce_limit=int(b), seed=0x3E5E000 + 7919 * salt + 977 * int(seed) + (1 if lens else 0), use_dof=bool(lens))


def _small_spheres(rng, n, lo=(-1.2, -0.8, 0.8), hi=(1.2, 0.8, 2.4), radius=(0.03, 0.12)):
    return [Object(Sphere(tuple(rng.uniform(lo, hi)), float(rng.uniform(*radius))), _material(rng)) for _ in range(n)]


def _scene(objs):
    sc = Scene()
    sc.objects = list(objs)
    return sc


# ---------------------------------------------------------------- the classes
def shared_grid(seed, lens=False):
    """Seeds 0, 1: two objects with different materials use ONE AccGrid — n_grids == 1 and n_grid_objects == 2, so no walk may be put aside (the
    carried state is one walk's) although there is one grid.  Seeds 2, 3: two grids built separately from the SAME mesh arrays, at the same
    place, with different materials.  Either way every grid hit is an exact distance tie between two objects and the lower index wins."""
    rng = np.random.default_rng([21, seed])
    lo, hi = _bounds(rng)
    mesh = _lumpy(4 + seed % 2, (1.5, 1.25, 0.75), (0.125, -0.125, 2.0))
    g1 = _grid(mesh)
    g2 = g1 if seed < 2 else _grid(Mesh(mesh.tri_pos, mesh.tri_nrm))
    twins = [Object(g1, _diffuse(rng)), Object(g2, _metal(rng))]
    if seed % 2:
        twins.reverse()
    scene = _shuffled(rng, _lit_room(rng, lo, hi, _kw(seed, lens, salt=1)["bounce_limit"]), twins + _small_spheres(rng, 2, radius=(0.1, 0.3)), ss._orders(seed))
    return scene, _camera(lens=lens), _kw(seed, lens, salt=1), "%s, room %s..%s" % ("one AccGrid in two objects" if seed < 2 else "two grids of one mesh", lo, hi)


GRID_POSITIONS = ((0,), ("last",), (63,), (64,), (70,), (62, 66))


def grid_positions(seed, lens=False):
    """GRID_POSITIONS[seed]: the grid object is object 0, the last object, object 63, 64 or 70 behind small filler spheres (visit_mask and
    grid_mask reach object 63; next_turn counts on from there), or two grid objects lie one on each side of index 64.  The walls are shuffled
    among the fillers."""
    rng = np.random.default_rng([22, seed])
    lo, hi = _bounds(rng)
    where = GRID_POSITIONS[seed % len(GRID_POSITIONS)]
    meshes = [_lumpy(4, (1.0, 1.0, 0.75), (-0.5, 0.0, 2.0)), _lumpy(3, (0.75, 1.0, 0.5), (0.625, 0.125, 1.75))]
    grids = [Object(_grid(meshes[i]), (_metal, _diffuse)[i](rng)) for i in range(len(where))]
    n_fill = 3 if where[0] in (0, "last") else max(where) + 3 - 6 - len(where)
    rest = [w[0] for w in _lit_room(rng, lo, hi, _kw(seed, salt=2)["bounce_limit"])] + _small_spheres(rng, n_fill)
    objs = [rest[i] for i in rng.permutation(len(rest))]
    for k, g in zip(where, grids):
        objs.insert(len(objs) if k == "last" else k, g)
    scene = _scene(objs)
    at = [i for i, o in enumerate(scene.objects) if isinstance(o.geometry, Grid)]
    assert at == [len(objs) - 1 if k == "last" else k for k in where]
    return scene, _camera(), _kw(seed, salt=2), "%d objects, grids at %s" % (len(objs), at)


def three_grids(seed, lens=False):
    """Three grid objects of three grids, interleaved with the room: three occupancy masks share the LDS budget.  Seeds 2, 3 are created under
    RMD_TUNE_MASK_BUDGET = 256 (scene_tunables): 256 bytes divided by three leave 21 words a grid — 640 cells at one bit each, fewer than any of
    these grids has up to its last non-empty cell — so mask_shift > 0 for each."""
    rng = np.random.default_rng([23, seed])
    lo, hi = _bounds(rng)
    meshes = [_lumpy(7, (0.875, 1.0, 0.75), (-0.875, 0.0, 2.0)), _lumpy(8, (0.75, 1.25, 0.5), (0.0, -0.125, 2.25)),
              gm.soup(rng, 700, lo=(0.5, -0.5, 1.5), hi=(1.25, 0.5, 2.25), spread=0.08)]
    grids = [Object(_grid(m), mat(rng)) for m, mat in zip(meshes, (_metal, _diffuse, _diffuse))]
    scene = _shuffled(rng, _lit_room(rng, lo, hi, _kw(seed, salt=3)["bounce_limit"]), grids + _small_spheres(rng, 1, radius=(0.1, 0.2)), ss._orders(seed))
    return scene, _camera(), _kw(seed, salt=3), "three grids%s" % (", mask budget 256" if seed >= 2 else "")


def camera_in_box(seed, lens=False):
    """The camera strictly inside the grid's bounding box, among a sparse soup (0); inside a closed mesh (1); one camera coordinate exactly ON
    a face of the box — soup(corners=True) makes the bounds the dyadic box itself — the near z face (2), the max x face (3)."""
    rng = np.random.default_rng([24, seed])
    lo, hi = _bounds(rng)
    which = seed % 4
    if which == 1:
        mesh, mat = _lumpy(5, (2.5, 1.75, 1.75), (0.0, 0.0, 0.25)), _metal(rng)
        others = [Object(Sphere((0.25, 0.25, 0.5), 0.25), _emission(rng))]  # light inside the mesh
    else:
        box = {0: ((-1.5, -1.0, -0.5), (1.5, 1.0, 1.25)), 2: ((-1.0, -0.75, 0.0), (1.0, 0.75, 1.5)), 3: ((-1.5, -1.0, 0.5), (0.0, 1.0, 2.0))}[which]
        mesh, mat = gm.soup(rng, 150, lo=box[0], hi=box[1], spread=0.06, corners=True), _diffuse(rng)
        others = _small_spheres(rng, 2, radius=(0.1, 0.25))
    scene = _shuffled(rng, _lit_room(rng, lo, hi, (1, 5, 5, 16)[which]), [Object(_grid(mesh), mat)] + others, ss._orders(seed))
    note = ("inside the box", "inside a closed mesh", "camera z is the box's near face", "camera x is the box's max face")[which]
    return scene, _camera(lens=lens), _kw(seed, lens, bounce_limit=(1, 5, 5, 16)[which], salt=4), note


CAMERA_ON_WALL_SEEDS = (0, 1, 6, 7)  # sphere_scenes.CAMERA_ON_WALLS: on the +x wall at bounce limit 16, on the -y wall, on a black wall, on a Diffuse one at limit 1


def camera_on_wall_with_mesh(seed, lens=False):
    """The room and camera of sphere_scenes.camera_on_walls (its seed CAMERA_ON_WALL_SEEDS[seed]) with a mesh in it: axis_pair_test's
    zero-numerator ballot, shade_last_depth and on_plane (api.cpp: make_params) in a launch with a grid.  Samples that face the wall are NaN."""
    inner = CAMERA_ON_WALL_SEEDS[seed % len(CAMERA_ON_WALL_SEEDS)]
    scene, cam, kw, note = ss.camera_on_walls(inner)
    rng = np.random.default_rng([25, seed])
    k, which, _ = ss.CAMERA_ON_WALLS[inner]
    extent, centre = (1.0, 0.75, 0.5), [cam.transform.position[0], cam.transform.position[1], 1.5]
    centre[k] += (extent[k] / 2.0 + 0.125) * (1.0 if which == "plus" else -1.0)  # beside the camera's wall, inside the room and in the view
    scene.objects.insert(int(rng.integers(0, len(scene.objects) + 1)), Object(_grid(_lumpy(4, extent, centre)), _metal(rng)))
    return scene, _camera(cam.transform.position), _kw(seed, bounce_limit=kw["bounce_limit"], salt=5), note + ", a mesh"


def no_ray_enters(seed, lens=False):
    """The mesh is behind the camera.  Seeds 0, 1 (the open variant): no plane, and in front of the camera only Emission spheres, where paths
    end — no ray of the frame enters the box: GEN and SHADE trips run alone.  Seeds 2, 3: in a room, where only bounce rays reach the mesh: the
    WALK trips start late and are never full."""
    rng = np.random.default_rng([26, seed])
    mesh = _lumpy(4, (2.5, 1.75, 0.75), (0.0, 0.0, -1.5))
    grid = Object(_grid(mesh), _diffuse(rng))
    if seed < 2:
        lights = [Object(Sphere((rng.uniform(-1.0, 1.0), rng.uniform(-0.6, 0.6), rng.uniform(1.5, 3.0)), float(rng.uniform(0.2, 0.5))), _emission(rng)) for _ in range(4)]
        objs = lights + [grid]
        return _scene([objs[i] for i in rng.permutation(len(objs))]), _camera(), _kw(seed, salt=6), "open: emitting spheres ahead, the mesh behind"
    lo, hi = _bounds(rng, lo_z=-2.5)
    mats = ss._wall_materials(rng)
    mats[3], mats[5] = _emission(rng), _diffuse(rng)  # the ceiling lights the room; the far wall, which most primary rays meet, sends them back
    scene = _shuffled(rng, _room(rng, lo, hi, mats), [grid] + _small_spheres(rng, 2, radius=(0.1, 0.3)), ss._orders(seed))
    return scene, _camera(), _kw(seed, bounce_limit=(5, 16)[seed % 2], salt=6), "a room, the mesh behind the camera"


def every_ray_walks(seed, lens=False):
    """The box fills the view.  Seeds 0, 1: a sparse soup — every primary ray is pushed or held as a ray and most walks find nothing; seeds 2,
    3: a dense closed mesh — most walks hit."""
    rng = np.random.default_rng([27, seed])
    lo, hi = [-3.0, -2.0, -1.0], [3.0, 2.5, 4.0]
    if seed < 2:
        mesh = gm.soup(rng, 60, lo=(-2.0, -1.5, 1.0), hi=(2.0, 1.5, 2.5), spread=0.03)
    else:
        mesh = _lumpy(6, (4.0, 3.0, 1.5), (0.0, 0.0, 2.0))
    scene = _shuffled(rng, _room(rng, lo, hi), [Object(_grid(mesh), _diffuse(rng) if seed % 2 else _metal(rng))], ss._orders(seed))
    return scene, _camera(lens=lens), _kw(seed, lens, bounce_limit=(5, 2, 16, 5)[seed % 4], salt=7), "the box fills the view: %s" % ("a sparse soup" if seed < 2 else "a closed mesh")


def mirror_box(seed, lens=False):
    """A closed low-roughness Metal mesh around the camera at bounce limit 16, with an emitting patch (a small Emission sphere inside): paths
    live to the limit — the depth byte and the RNG block counter of the packed queue words, the longest trip sequences."""
    rng = np.random.default_rng([28, seed])
    mesh = _lumpy(5 + seed % 2, (3.0, 2.0, 2.0), (0.0, 0.0, 0.5))
    col = tuple(rng.uniform(0.85, 1.0, 3))
    objs = [Object(_grid(mesh), Material.Metal(col, (0.03, 0.01)[seed % 2])), Object(Sphere((0.5, 0.375, 0.75), 0.375), _emission(rng))]
    if seed % 2:
        objs.reverse()
    return _scene(objs), _camera(lens=lens), _kw(seed, lens, bounce_limit=16, salt=8), "a mirror mesh around the camera"


ONE_CELL = ("single", "scan_r0", "scan_r1")  # resolutions (1, 1, 1), (2, 1, 1), (3, 1, 1)
FEW_CELLS = ("few", "scan_r3", "cluster", "spanning")  # 2^3 and 3^3 cells; 20^3 with a run of 512 / 513 in one cell: many full chunks in one walk


def _unit_mesh_scene(name, rng, seed, salt):
    mesh = _adversarial()[name]
    size = mesh.tri_pos.reshape(-1, 3).max(axis=0)
    mesh = _moved(mesh, (-size[0] / 2.0, -0.5, 1.5))  # (dyadic: the unit meshes' bounds are whole numbers)
    lo, hi = _bounds(rng)
    scene = _shuffled(rng, _lit_room(rng, lo, hi, _kw(seed, salt=salt)["bounce_limit"]), [Object(_grid(mesh), _material(rng))] + _small_spheres(rng, 2, radius=(0.1, 0.2)), ss._orders(seed))
    return scene, _camera(), _kw(seed, salt=salt), "grid_meshes' %s" % name


def one_cell(seed, lens=False):
    """grid_meshes' single, scan_r0 and scan_r1 as scene geometry: one cell, and a row of two or three (walk_steps_bound 6 to 8)."""
    return _unit_mesh_scene(ONE_CELL[seed % len(ONE_CELL)], np.random.default_rng([29, seed]), seed, 9)


def few_cells(seed, lens=False):
    """grid_meshes' few and scan_r3 (8 and 27 cells), and cluster and spanning: runs of hundreds in one cell."""
    return _unit_mesh_scene(FEW_CELLS[seed % len(FEW_CELLS)], np.random.default_rng([30, seed]), seed, 10)


FLAT = 2.0 ** -5  # the thinnest box 4,096 triangles build a grid for (its resolution on that axis is 1); at 2**-20 the resolution is zero and no grid builds


def thin_and_flat(seed, lens=False):
    """A nearly flat mesh (a box of zero extent cannot build): a soup in a box FLAT thin, facing the camera (seed 0: thin on z) and edge-on
    (seed 1: thin on x, at the camera's x)."""
    rng = np.random.default_rng([31, seed])
    lo, hi = _bounds(rng)
    if seed % 2 == 0:
        mesh = gm.soup(rng, 4096, lo=(-1.0, -0.75, 2.0), hi=(1.0, 0.75, 2.0 + FLAT), spread=0.03)
    else:
        mesh = gm.soup(rng, 4096, lo=(0.0, -1.0, 1.0), hi=(FLAT, 1.0, 2.5), spread=0.03)
    scene = _shuffled(rng, _lit_room(rng, lo, hi, _kw(seed, salt=11)["bounce_limit"]), [Object(_grid(mesh), _diffuse(rng))] + _small_spheres(rng, 1, radius=(0.1, 0.2)), ss._orders(seed))
    return scene, _camera(), _kw(seed, salt=11), "a soup %g thin, %s" % (FLAT, "facing the camera" if seed % 2 == 0 else "edge-on")


MATERIALS = ("emission", "black", "roughness-0")


def materials(seed, lens=False):
    """An Emission mesh (0), a black Diffuse mesh (1) and a roughness-0 Metal mesh (2: the irregular case, NaN for NaN); each is rendered with
    flags 0, RMD_RENDER_TRACE_BLACK_PATHS and RMD_RENDER_END_BLACK_PATHS (render_flags)."""
    rng = np.random.default_rng([32, seed])
    lo, hi = _bounds(rng)
    mat = (_emission(rng), _black(rng), Material.Metal((1.0, 0.9, 0.8), 0.0))[seed % 3]
    mesh = _lumpy(5, (1.5, 1.25, 0.75), (0.0, 0.0, 2.0))
    scene = _shuffled(rng, _lit_room(rng, lo, hi, _kw(seed, salt=12)["bounce_limit"]), [Object(_grid(mesh), mat)] + _small_spheres(rng, 2, radius=(0.1, 0.3)), ss._orders(seed))
    return scene, _camera(), _kw(seed, salt=12), "a mesh of %s" % MATERIALS[seed % 3]


def nan_normals(seed, lens=False):
    """grid_meshes' nan_vertex (0: one NaN coordinate, which the bounds skip and the triangle test meets) and a closed mesh whose vertex
    normals are NaN at every seventh triangle (1).  Samples may be NaN, compared NaN for NaN."""
    rng = np.random.default_rng([33, seed])
    lo, hi = _bounds(rng)
    if seed % 2 == 0:
        mesh = _moved(_adversarial()["nan_vertex"], (-0.5, -0.5, 1.5))
    else:
        mesh = _lumpy(5, (1.5, 1.25, 0.75), (0.0, 0.0, 2.0))
        mesh.tri_nrm[::7] = np.nan
    scene = _shuffled(rng, _room(rng, lo, hi), [Object(_grid(mesh), _diffuse(rng) if seed % 2 else _metal(rng))], ss._orders(seed))
    return scene, _camera(), _kw(seed, bounce_limit=5, salt=13), "NaN %s" % ("in a vertex" if seed % 2 == 0 else "normals")


def open_scene(seed, lens=False):
    """A mesh and spheres with no plane at all (axis_pairs == 0): most paths end on a miss."""
    rng = np.random.default_rng([34, seed])
    mesh = _lumpy(5, (1.25, 1.0, 0.75), (-0.25, 0.0, 2.0))
    objs = [Object(_grid(mesh), _metal(rng) if seed % 2 else _diffuse(rng)), Object(Sphere((0.0, 3.0, 2.0), 1.5), _emission(rng))]
    objs += _small_spheres(rng, 4, radius=(0.1, 0.35))
    return _scene([objs[i] for i in rng.permutation(len(objs))]), _camera(), _kw(seed, salt=14), "no plane: a mesh, a light and four spheres"


def partial_room_with_mesh(seed, lens=False):
    """sphere_scenes.partial_room (one or two axis pairs, the planes shuffled among the other objects) with a grid object as object 0 (even
    seeds: every pair's later plane sits above the grid's index) or as the last object (odd seeds: below it)."""
    scene, cam, kw, note = ss.partial_room(seed)
    rng = np.random.default_rng([35, seed])
    grid = Object(_grid(_lumpy(4, (1.0, 0.75, 0.5), (0.25, -0.125, 1.75))), _material(rng))
    scene.objects.insert(0 if seed % 2 == 0 else len(scene.objects), grid)
    return scene, _camera(), _kw(seed, bounce_limit=(16, 5, 2, 5)[seed % 4], salt=15), note + ", the grid %s" % ("first" if seed % 2 == 0 else "last")


CLASSES = {f.__name__: f for f in (shared_grid, grid_positions, three_grids, camera_in_box, camera_on_wall_with_mesh, no_ray_enters, every_ray_walks,
                                   mirror_box, one_cell, few_cells, thin_and_flat, materials, nan_normals, open_scene, partial_room_with_mesh)}
SEEDS = {"shared_grid": (0, 1, 2, 3), "grid_positions": tuple(range(len(GRID_POSITIONS))), "three_grids": (0, 1, 2, 3), "camera_in_box": (0, 1, 2, 3),
         "camera_on_wall_with_mesh": tuple(range(len(CAMERA_ON_WALL_SEEDS))), "no_ray_enters": (0, 1, 2, 3), "every_ray_walks": (0, 1, 2, 3),
         "mirror_box": (0, 1), "one_cell": tuple(range(len(ONE_CELL))), "few_cells": tuple(range(len(FEW_CELLS))), "thin_and_flat": (0, 1),
         "materials": (0, 1, 2), "nan_normals": (0, 1), "open_scene": (0, 1), "partial_room_with_mesh": (0, 1, 2, 3)}
LENS_CLASSES = ("shared_grid", "camera_in_box", "every_ray_walks", "mirror_box")
LENS_SEEDS = {"shared_grid": (0, 2), "camera_in_box": (0, 1), "every_ray_walks": (0, 2), "mirror_box": (0, 1)}  # the seeds whose thin-lens variant is yielded
NAN_FOR_NAN = ("camera_on_wall_with_mesh", "materials", "nan_normals")  # classes whose samples may be NaN: frames compare NaN for NaN


def cases(classes=None, lens=None):
    """[(class, seed, lens)] — every class and seed, and the thin-lens variants; lens=False / True keeps one kind"""
    out = []
    for name in classes or CLASSES:
        out += [(name, s, False) for s in SEEDS[name]]
        if name in LENS_CLASSES:
            out += [(name, s, True) for s in LENS_SEEDS[name]]
    return [c for c in out if lens is None or c[2] == lens]


def case_id(case):
    return "%s-%d%s" % (case[0], case[1], "-lens" if case[2] else "")


@functools.lru_cache(maxsize=None)
def _built(case):
    return CLASSES[case[0]](case[1], lens=case[2])


def build(case, **flags):
    """-> (Scene, CameraSettings, Settings, note); the scene is built once per process and shared: read it, do not change it.  flags: further
    Settings keywords (one of render_flags(case))"""
    scene, cam, kw, note = _built(tuple(case))
    return scene, cam, Settings(cam, **dict(kw, **flags)), note


def scene_tunables(case):
    """{tunable: value} the case's DeviceScene is created under"""
    return {abi.RMD_TUNE_MASK_BUDGET: 256} if case[0] == "three_grids" and case[1] >= 2 else {}


def render_flags(case):
    """the black-path modes a case is rendered with besides flags 0, as Settings keywords"""
    return (dict(trace_black_paths=True), dict(end_black_paths=True)) if case[0] == "materials" else ()


# ---------------------------------------------------------------- plain geometry, for the self-checks
def grid_objects(scene):
    return [i for i, o in enumerate(scene.objects) if isinstance(o.geometry, Grid)]


def distinct_grids(scene):
    out = []
    for o in scene.objects:
        if isinstance(o.geometry, Grid) and not any(o.geometry.grid is g for g in out):
            out.append(o.geometry.grid)
    return out


def primary_directions(cam):
    """the pinhole directions through the pixel centres, unnormalised (x, y, 1) — enough for which boxes the frame's primary rays can enter"""
    W, H = cam.backbuffer_width, cam.backbuffer_height
    ey = math.tan(math.radians(cam.fov_vert) / 2.0)
    ex = ey * W / H
    xs, ys = (np.arange(W) + 0.5) / W * 2.0 - 1.0, 1.0 - (np.arange(H) + 0.5) / H * 2.0
    d = np.stack(np.broadcast_arrays(xs[None, :] * ex, ys[:, None] * ey, np.ones((H, W))), axis=2).reshape(-1, 3)
    return d


def rays_entering(grid, origin, d):
    """the slab test on the grid's box for rays from `origin`: tmax > max(tmin, 0)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (np.asarray(grid.bbox_min) - np.asarray(origin)) / d
        t2 = (np.asarray(grid.bbox_max) - np.asarray(origin)) / d
    tmin, tmax = np.fmin(t1, t2).max(axis=1), np.fmax(t1, t2).min(axis=1)
    return tmax > np.maximum(tmin, 0.0)
