"""Adversarial scenes for the grid-less render kernel (render_kernel.hpp: render_wave_sorted / render_wave) — plain numpy, no GPU, no oracle.

Every form-against-form test of the spheres kernel used to render one world: the six-wall room of scenes.reflective_spheres(), the camera of
scenes.camera() strictly inside it, 32x32 host tiles on the 8-pixel lattice.  What the kernel decides once per scene or per tile —
rmd::derive_scene_objects (which planes pair, which pairs become axis pairs, the 10-bit field per axis, visit_mask, `regular`), axis_pair_test's
fast path and its ballot, the generation trips' candidate sets, the two hit stacks — was seen in one state.  The classes below put each of those
decisions into its other states.  tests/test_sphere_scenes_host.py holds the oracle to the second reading of the source on every class (which is
what makes the oracle's answer a reference for them) and asserts through the host probe that a class exercises what it names;
tests/test_gpu_sphere_scenes.py then holds every launch form of the device to form A byte for byte, and to the oracle.

Twelve classes are aimed at the scene table and the candidate sets: shuffled_room, signed_zero_normals, partial_room, duplicate_walls, tilted_pairs,
camera_on_walls, coincident_spheres, table_edges, one_lobe, rough_extremes, fov_and_aspect, irregular.  Five (TILE_CLASS_CLASSES) are aimed at the
TILE CLASSES of primary_candidates.hpp — the work items that see one wall and end their samples as an EMITTER or a BLACK item, which the twelve
barely reach: one_wall_mixed (EMITTER, BLACK and general tiles in one frame, bounce limits 1, 2, 5, 16; with a thin-lens variant),
emitter_colours (every tile EMITTER; signed zeros, denormals, a negative component, 1e150), black_walls (every tile BLACK; the wall's colour as
signed zeros, roughness 512 and 1e-12, first and last in the table, a black Metal wall that must stay general), class_table_edge (63, 64 and 65
objects: the last table length with classes and the first without) and ragged_one_wall (frames from 1x1 to 41x25: classed tiles one pixel wide
and high).

One function per class, seeded and deterministic: f(seed, lens=False) -> (Scene, CameraSettings, dict of Settings keywords, note).  CLASSES names
them, SEEDS gives each class's seeds (at least two), LENS_CLASSES the classes that also yield a thin-lens variant (use_dof with C5's aperture:
the candidate sets must switch themselves off).  cases() lists (class, seed, lens); build(case) makes one.

Deliberate coincidences are EXACT, never near: identical copies of an object share the same Python floats, wall coordinates are dyadic (multiples
of 1/8), a camera coordinate that sits on a wall IS the wall's coordinate as the same double.  Both sides then meet the same tie and no libm ulp
decides a hit.  Every scene is one rmd_scene_create accepts: |roughness| <= 512, and no 0 < |roughness| < 1e-12.

The room's convention: the wall with normal +e_k lies at lo[k] (AxisWalls::o_plus), the one with normal -e_k at hi[k] (o_minus); a camera is
strictly inside on axis k when lo[k] < position[k] < hi[k].  The camera has no rotation: it looks down +z.
"""
import math

import numpy as np

from raymond_amd import abi
from raymond_amd.scene import CameraSettings, Material, Object, Plane, Scene, Settings, Sphere, Transform

SPP = 160  # >= kSortedMinSamples (128): the automatic launch is the role-sorted one
FRAME = (40, 24)  # 15 wave tiles, ragged
APERTURE = 0.5  # C5's, as tests/test_gpu_lobe_trips.py's thin-lens case
BOUNCE_LIMITS = (1, 2, 5, 16)
THOUSAND_FRAME, THOUSAND_SPP = (16, 16), 130  # the thousand-object rooms of table_edges: the oracle's render stays at seconds


# ---------------------------------------------------------------- parts
def _dyadic(rng, lo, hi):
    """a multiple of 1/8 in [lo, hi]"""
    return float(rng.integers(int(round(lo * 8)), int(round(hi * 8)) + 1)) / 8.0


def _bounds(rng):
    """(lo, hi) of a room around the origin, dyadic; the far wall near enough that the middle tiles keep the z pair alone"""
    lo = [-_dyadic(rng, 1.5, 3.0), -_dyadic(rng, 1.0, 2.0), -_dyadic(rng, 0.5, 2.0)]
    hi = [_dyadic(rng, 1.5, 3.0), _dyadic(rng, 1.0, 2.5), _dyadic(rng, 2.5, 4.5)]
    return lo, hi


def _diffuse(rng):
    return Material.Diffuse(tuple(rng.uniform(0.2, 0.95, 3)), float(rng.uniform(0.05, 0.9)))


def _black(rng):
    return Material.Diffuse((0.0, 0.0, 0.0), float(rng.uniform(0.1, 0.9)))


def _metal(rng):
    return Material.Metal(tuple(rng.uniform(0.3, 1.0, 3)), float(rng.uniform(0.02, 0.4)))


def _emission(rng):
    e = float(rng.uniform(0.8, 2.5))
    return Material.Emission((e, e * float(rng.uniform(0.7, 1.0)), e * float(rng.uniform(0.5, 1.0))))


def _material(rng):
    return (_diffuse, _diffuse, _metal, _metal, _black, _emission)[int(rng.integers(0, 6))](rng)


def _wall_materials(rng, n=6):
    """an emitting and a black wall among them, the rest drawn"""
    mats = [_emission(rng), _black(rng)] + [_material(rng) for _ in range(n - 2)]
    return [mats[i] for i in rng.permutation(n)]


def _wall(k, plus, coord, rng=None, off_axis=False, neg_zero=False, length=1.0):
    """the plane with normal +e_k (plus) or -e_k at coordinate `coord` of axis k; off_axis: the origin's other components are arbitrary;
    neg_zero: the normal's zero components are -0.0 or +0.0 by a coin each"""
    n = [0.0, 0.0, 0.0]
    o = [0.0, 0.0, 0.0]
    if off_axis:
        o = [float(v) for v in rng.uniform(-5.0, 5.0, 3)]
    if neg_zero:
        n = [-0.0 if int(rng.integers(0, 2)) else 0.0 for _ in range(3)]
    n[k] = length if plus else -length
    o[k] = coord
    return Plane(o, n)


def _room(rng, lo, hi, mats=None, **how):
    """the six walls as [(Object, axis, plus)]"""
    mats = mats or _wall_materials(rng)
    out = []
    for k in range(3):
        out.append((Object(_wall(k, True, lo[k], rng, **how), mats[2 * k]), k, True))
        out.append((Object(_wall(k, False, hi[k], rng, **how), mats[2 * k + 1]), k, False))
    return out


def _spheres(rng, lo, hi, n, radius=(0.1, 0.6)):
    out = []
    for _ in range(n):
        c = (rng.uniform(0.8 * lo[0], 0.8 * hi[0]), rng.uniform(0.8 * lo[1], 0.8 * hi[1]), rng.uniform(1.0, hi[2]))
        out.append(Object(Sphere(c, float(rng.uniform(*radius))), _material(rng)))
    return out


def _shuffled(rng, walls, others, plus_first):
    """one object list: walls and others in random order, the two walls of axis k in the order plus_first[k] asks for"""
    items = [w[0] for w in walls] + list(others)
    order = [int(i) for i in rng.permutation(len(items))]
    slot = {i: s for s, i in enumerate(order)}  # item -> position
    for k in range(3):
        pair = [i for i, w in enumerate(walls) if w[1] == k]
        if len(pair) != 2:
            continue
        p, m = (pair[0], pair[1]) if walls[pair[0]][2] else (pair[1], pair[0])
        if (slot[p] < slot[m]) != bool(plus_first[k]):
            slot[p], slot[m] = slot[m], slot[p]
    scene = Scene()
    scene.objects = [items[i] for i in sorted(slot, key=slot.get)]
    return scene


def _camera(pos=(0.0, 0.0, 0.0), frame=FRAME, fov=55.0, lens=False):
    return CameraSettings(frame[0], frame[1], fov, Transform(tuple(float(v) for v in pos)), focal_length=2.5, aperture_radius=APERTURE if lens else 0.0)


def _kw(rng, seed, lens=False, bounce_limit=None, spp=SPP):
    b = BOUNCE_LIMITS[int(rng.integers(0, 4))] if bounce_limit is None else bounce_limit
    return dict(sample_count=spp, tile_size=(32, 32), bounce_limit=int(b), seed=0x5CE7E000 + 977 * int(seed) + (1 if lens else 0), use_dof=bool(lens))


def _orders(seed):
    """which wall of each axis comes first: both kinds in every scene, another assignment per seed"""
    return [(seed + k) % 2 == 0 for k in range(3)]


# ---------------------------------------------------------------- the classes
def shuffled_room(seed, lens=False):
    """Six axis walls at random dyadic coordinates, in random object order, interleaved with 0 - 6 spheres (seed 0: none, seed 1: six); on some
    axes the +e_k wall comes first, on others the -e_k wall; an emitting and a black wall.  Aimed at kObjAxisEarlierIsPlus, AxisWalls and
    visit_mask with walls anywhere."""
    rng = np.random.default_rng([1, seed])
    lo, hi = _bounds(rng)
    n = (0, 6, 3, 1)[seed % 4]
    scene = _shuffled(rng, _room(rng, lo, hi), _spheres(rng, lo, hi, n), _orders(seed))
    return scene, _camera(lens=lens), _kw(rng, seed, lens), "room %s..%s, %d spheres" % (lo, hi, n)


def signed_zero_normals(seed, lens=False):
    """shuffled_room's room with -0.0 in the zero components of some normals and arbitrary off-axis components in the plane origins: the
    "same bits" argument of axis_pair_test (x + (+-0) = x)."""
    rng = np.random.default_rng([2, seed])
    lo, hi = _bounds(rng)
    n = (2, 0, 5)[seed % 3]
    scene = _shuffled(rng, _room(rng, lo, hi, off_axis=True, neg_zero=True), _spheres(rng, lo, hi, n), _orders(seed + 1))
    assert any(math.copysign(1.0, c) < 0.0 and c == 0.0 for o in scene.objects if isinstance(o.geometry, Plane) for c in o.geometry.normal)
    return scene, _camera(), _kw(rng, seed), "signed zeros in the walls' normals, %d spheres" % n


def partial_room(seed, lens=False):
    """One or two axis pairs only, single unpaired axis planes and one or two tilted planes; some directions are open, so paths miss: a
    generation trip whose lanes partly end, stacks that receive fewer than 64 hits; primary_pairs_kept with unpaired axes."""
    rng = np.random.default_rng([3, seed])
    lo, hi = _bounds(rng)
    paired = ([1], [0, 1], [1, 2], [0])[seed % 4]
    mats = _wall_materials(rng, 10)
    walls, singles = [], []
    for k in range(3):
        if k in paired:
            walls.append((Object(_wall(k, True, lo[k]), mats[2 * k]), k, True))
            walls.append((Object(_wall(k, False, hi[k]), mats[2 * k + 1]), k, False))
        elif int(rng.integers(0, 3)) or k == 2:  # a single wall of this axis (always one on z, behind the scene or behind the camera)
            plus = bool(rng.integers(0, 2))
            singles.append(Object(_wall(k, plus, lo[k] if plus else hi[k]), mats[2 * k]))
    for t in range(1 + seed % 2):  # tilted planes below / beside the view, facing it
        nrm = np.array([rng.uniform(-0.4, 0.4), 1.0, rng.uniform(-0.4, 0.1)]) if t == 0 else np.array([1.0, rng.uniform(-0.3, 0.3), rng.uniform(-0.5, 0.0)])
        nrm = nrm / np.sqrt((nrm * nrm).sum())
        org = (0.0, lo[1] - 0.25, 2.0) if t == 0 else (lo[0] - 0.25, 0.0, 2.0)
        singles.append(Object(Plane(org, nrm), mats[6 + t]))
    singles.append(Object(Sphere((0.0, hi[1] + 1.0, 2.0), 0.75), _emission(rng)))  # light from above whatever the walls' materials
    scene = _shuffled(rng, walls, singles + _spheres(rng, lo, hi, 2), _orders(seed))
    return scene, _camera(lens=lens), _kw(rng, seed, lens), "axis pairs on %s, %d other planes" % (paired, len(singles) - 1)


def duplicate_walls(seed, lens=False):
    """On x two complete pairs (inner and outer); on y three planes of normal +e_y at three heights and one of -e_y; on z a pair and an
    IDENTICAL copy (the same doubles, another material) of its -e_z wall.  One pair per axis becomes an axis pair and the rest stay general;
    the copy ties exactly with the original and the first object wins (lex_less)."""
    rng = np.random.default_rng([4, seed])
    lo, hi = _bounds(rng)
    mats = _wall_materials(rng, 12)
    mats[7] = _emission(rng)  # the ceiling: the one -e_y plane, which no other plane hides
    back = _wall(2, False, hi[2])
    planes = [_wall(0, True, lo[0]), _wall(0, False, hi[0]), _wall(0, True, lo[0] - 0.5), _wall(0, False, hi[0] + 0.5),
              _wall(1, True, lo[1]), _wall(1, True, lo[1] - 0.25), _wall(1, True, lo[1] + 0.125), _wall(1, False, hi[1]),
              _wall(2, True, lo[2]), back, Plane(back.origin, back.normal)]
    objs = [Object(p, mats[i]) for i, p in enumerate(planes)] + _spheres(rng, lo, hi, 2)
    scene = Scene()
    scene.objects = [objs[i] for i in rng.permutation(len(objs))]
    return scene, _camera(), _kw(rng, seed, bounce_limit=(5, 16)[seed % 2]), "two x pairs, 3 + 1 y planes, a copied z wall"


def tilted_pairs(seed, lens=False):
    """A room whose walls are pairs of opposite NON-axis normals (a rotated box), some not of unit length, and on one axis normals +-2 e_k:
    every pair goes through plane_pair_test_flat (kPairTestedAtPartner), none through the axis rule."""
    rng = np.random.default_rng([5, seed])
    lo, hi = _bounds(rng)
    a, b = rng.uniform(0.1, 0.5, 2)
    ca, sa, cb, sb = math.cos(a), math.sin(a), math.cos(b), math.sin(b)
    rot = np.array([[ca, 0.0, sa], [0.0, 1.0, 0.0], [-sa, 0.0, ca]]) @ np.array([[1.0, 0.0, 0.0], [0.0, cb, -sb], [0.0, sb, cb]])
    mats = _wall_materials(rng)
    objs = []
    centre = np.array([0.0, 0.0, 1.0])
    for k in range(3):
        if k == seed % 3:  # axis-aligned, but of length 2: no axis pair (the rule wants exactly +-1)
            n_plus, o_plus, o_minus = np.eye(3)[k] * 2.0, np.eye(3)[k] * lo[k], np.eye(3)[k] * hi[k]
        else:
            length = (1.0, 0.5, 3.0)[(seed + k) % 3]
            n_plus = rot[:, k] * length
            o_plus, o_minus = centre + rot[:, k] * lo[k], centre + rot[:, k] * hi[k]
        objs.append(Object(Plane(o_plus, n_plus), mats[2 * k]))
        objs.append(Object(Plane(o_minus, [-float(v) for v in n_plus]), mats[2 * k + 1]))  # the exact negation
    objs += _spheres(rng, lo, [hi[0], hi[1], 2.5], 2)
    scene = Scene()
    scene.objects = [objs[i] for i in rng.permutation(len(objs))]
    return scene, _camera(), _kw(rng, seed), "rotated box, normal lengths 0.5 .. 3"


CAMERA_ON_WALLS = ((0, "plus", "on"), (1, "minus", "on"), (0, "minus", "inside"), (1, "plus", "outside"), (0, "plus", "far"), (2, "minus", "on"),
                   (0, "minus", "on"), (1, "plus", "on"))


def camera_on_walls(seed, lens=False):
    """A camera coordinate that is exactly a wall's (o_plus or o_minus, the same double), one nextafter step inside or outside of it, or half a
    unit outside the room: the zero-numerator ballot of axis_pair_test, primary_pairs_kept's "strictly inside".  CAMERA_ON_WALLS[seed] names
    (axis, wall, where).  A primary ray that faces the wall the camera sits on hits it at t = 0: the hit point IS the camera position, the view
    direction normalize(camera - hit) is NaN, and unless that wall emits the reference's sample is NaN.  Seed 6 makes that wall black Diffuse
    (a path the kernel would end as black) and seed 7 a coloured Diffuse at bounce limit 1 (a hit at the last depth): NaN for NaN there too."""
    rng = np.random.default_rng([6, seed])
    lo, hi = _bounds(rng)
    k, which, where = CAMERA_ON_WALLS[seed % len(CAMERA_ON_WALLS)]
    scene = _shuffled(rng, _room(rng, lo, hi), _spheres(rng, lo, hi, 2), _orders(seed))
    c = lo[k] if which == "plus" else hi[k]
    inward = math.inf if which == "plus" else -math.inf
    pos = [0.125, -0.125, 0.0]
    pos[k] = {"on": c, "inside": math.nextafter(c, inward), "outside": math.nextafter(c, -inward), "far": c - math.copysign(0.5, inward)}[where]
    bounces = (16, 2, 5, 2, 5, 2, 5, 1)[seed % len(CAMERA_ON_WALLS)]
    if seed % len(CAMERA_ON_WALLS) in (6, 7):
        wall = next(o for o in scene.objects if isinstance(o.geometry, Plane) and o.geometry.normal[k] != 0.0 and o.geometry.origin[k] == c)
        wall.material = _black(rng) if seed % len(CAMERA_ON_WALLS) == 6 else _diffuse(rng)
    return scene, _camera(pos, lens=lens), _kw(rng, seed, lens, bounce_limit=bounces), "camera %s: axis %d, the %s wall, %s" % (pos, k, which, where)


def camera_strictly_inside(scene, cam):
    """per axis: None without an axis-aligned pair in `scene`, else whether the camera lies strictly between the outermost +e_k / -e_k walls"""
    out = []
    for k in range(3):
        e = [0.0, 0.0, 0.0]
        e[k] = 1.0
        plus = [o.geometry.origin[k] for o in scene.objects if isinstance(o.geometry, Plane) and list(o.geometry.normal) == e]
        minus = [o.geometry.origin[k] for o in scene.objects if isinstance(o.geometry, Plane) and list(o.geometry.normal) == [-v for v in e]]
        out.append(None if not plus or not minus else max(plus) < cam.transform.position[k] < min(minus))
    return out


def coincident_spheres(seed, lens=False):
    """The same sphere at two indices with different materials; concentric spheres; a sphere that contains the camera; a sphere of radius 1e3
    that contains the room; one of radius 1e-3; spheres cut by walls (centre ON the wall's coordinate); a sphere beside the camera (in front of
    the tiles that look away from it, to the side of the others) and one behind it (90 degrees or more from every ray of the frame: the
    candidate sets need not recognise it, `in_front` is false on every tile and its bit stays — which is what a predicate that ignored
    `in_front` would get wrong without any frame showing it).  Ties, primary_sphere_cleared never clearing what is hit, sphere_test_flat from
    inside."""
    rng = np.random.default_rng([7, seed])
    lo, hi = _bounds(rng)
    twin = Sphere((_dyadic(rng, -1.0, -0.5), _dyadic(rng, -0.5, 0.5), _dyadic(rng, 2.0, 2.5)), 0.375)
    centre = (_dyadic(rng, 0.5, 1.0), _dyadic(rng, -0.5, 0.5), _dyadic(rng, 2.0, 2.5))
    spheres = [Object(twin, _diffuse(rng)), Object(Sphere(twin.origin, twin.radius), _metal(rng)),
               Object(Sphere(centre, 0.5), _diffuse(rng)), Object(Sphere(centre, 0.25), _emission(rng)),
               Object(Sphere((0.125, -0.125, 0.25), 0.5), _metal(rng)),  # contains the camera
               Object(Sphere((0.25, 0.5, 1.0), 1e3), _diffuse(rng)),  # contains the room
               Object(Sphere((0.25, 0.125, 1.5), 1e-3), _emission(rng)),
               Object(Sphere((lo[0], 0.25, 2.5), 0.5), _material(rng)), Object(Sphere((0.5, lo[1], 2.0), 0.5), _material(rng)),  # cut by walls
               Object(Sphere((1.5, 0.0, 0.0625), 0.25), _diffuse(rng)),  # beside the camera
               Object(Sphere((0.25, 0.125, -0.5), 0.25), _diffuse(rng))]  # behind it
    scene = _shuffled(rng, _room(rng, lo, hi), spheres, _orders(seed))
    return scene, _camera(lens=lens), _kw(rng, seed, lens), "eleven spheres in a room"


TABLE_EDGES = (("small", 57), ("small", 58), ("small", 59), ("small", 62), ("thousand", 1017), ("thousand", 1018), ("thousand", 1019), ("thousand", 1016))


def table_edges(seed, lens=False):
    """TABLE_EDGES[seed] = (kind, n): n small spheres FIRST, then the six walls.  small: 63, 64 and 65 objects (n = 57, 58, 59) and walls at
    62 .. 67 — visit_mask's reach, which ends at object 63.  thousand: the later planes of the three axis pairs have the indices n + 1, n + 3 and
    n + 5: with n = 1017 the last one is 1022, the 10-bit field's last value; with 1018 it is 1023, the first overflow (that pair stays general);
    with 1019 the second pair's is 1022 and the third's 1024.  Frame 16x16 at 130 spp there."""
    rng = np.random.default_rng([8, seed])
    kind, n = TABLE_EDGES[seed % len(TABLE_EDGES)]
    lo, hi = _bounds(rng)
    walls = [w[0] for w in _room(rng, lo, hi)]
    axes = [int(a) for a in rng.permutation(3)]  # which axis gets which place in the table
    flip = [bool(rng.integers(0, 2)) for _ in range(3)]
    walls = [walls[2 * a + (1 - i if flip[a] else i)] for a in axes for i in range(2)]
    scene = Scene()
    if kind == "small":
        scene.objects = _spheres(rng, lo, hi, n, radius=(0.03, 0.12)) + walls
        return scene, _camera(), _kw(rng, seed), "%d objects, the walls at %d .. %d" % (n + 6, n, n + 5)
    for _ in range(n):
        c = (rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6), rng.uniform(1.0, 2.0))
        scene.objects.append(Object(Sphere(c, float(rng.uniform(0.004, 0.03))), _material(rng)))
    scene.objects += walls
    kw = _kw(rng, seed, bounce_limit=(2, 5)[seed % 2], spp=THOUSAND_SPP)
    return scene, _camera(frame=THOUSAND_FRAME), kw, "%d objects, axis order %s, later planes at %d, %d, %d" % (n + 6, axes, n + 1, n + 3, n + 5)


def one_lobe(seed, lens=False):
    """Every object Emission (seed 0: no hit is ever parked), every object black Diffuse (1: every path ends at its first hit; the frame is
    black), every object Metal at bounce limit 16 (2: the diffuse stack stays empty and all paths run to the limit; the frame is black too, no
    object emits) and, so that such paths also carry radiance, every object Metal but one emitting wall (3)."""
    rng = np.random.default_rng([9, seed])
    lo, hi = _bounds(rng)
    make, bounces = ((_emission, 5), (_black, 5), (_metal, 16), (_metal, 16))[seed % 4]
    scene = _shuffled(rng, _room(rng, lo, hi), _spheres(rng, lo, hi, 2), _orders(seed))
    for o in scene.objects:
        o.material = make(rng)
    if seed % 4 == 3:
        next(o for o in scene.objects if isinstance(o.geometry, Plane) and o.geometry.normal[1] == -1.0).material = _emission(rng)
    return scene, _camera(), _kw(rng, seed, bounce_limit=bounces), "every object %s%s" % (make.__name__[1:], ", one emitting wall" if seed % 4 == 3 else "")


def rough_extremes(seed, lens=False):
    """Roughness 512 (the largest accepted) and 1e-12 (the smallest), on Diffuse and Metal, walls and spheres; colours above 1, so throughputs
    grow.  The GGX angle's reduction."""
    rng = np.random.default_rng([10, seed])
    lo, hi = _bounds(rng)
    scene = _shuffled(rng, _room(rng, lo, hi), _spheres(rng, lo, hi, 3), _orders(seed))
    rough = (512.0, 1e-12, -512.0, 512.0, 1e-12, 0.3)
    n = 0
    for o in scene.objects:
        m = o.material
        if m.kind == abi.RMD_MAT_EMISSION:
            continue
        r = rough[(n + seed) % len(rough)]
        color = m.color if m.color == (0.0, 0.0, 0.0) else tuple(float(c) * (1.0, 1.6, 3.0)[n % 3] for c in m.color)
        o.material = Material(m.kind, color, r, m.aux)
        n += 1
    return scene, _camera(), _kw(rng, seed, bounce_limit=(5, 16)[seed % 2]), "roughness in {512, -512, 1e-12}, colours up to 3"


FOV_AND_ASPECT = ((5.0, (97, 9)), (150.0, (9, 97)), (150.0, (97, 9)), (5.0, (9, 97)))


def fov_and_aspect(seed, lens=False):
    """fov_vert about 5 and about 150 degrees on frames 97x9 and 9x97 (FOV_AND_ASPECT[seed]): TileCone.ok false and true within one frame."""
    rng = np.random.default_rng([11, seed])
    lo, hi = _bounds(rng)
    fov, frame = FOV_AND_ASPECT[seed % len(FOV_AND_ASPECT)]
    fov = fov * float(rng.uniform(0.97, 1.03))
    others = _spheres(rng, lo, hi, 3)
    if fov < 10.0:  # something to see in so narrow a view
        others.append(Object(Sphere((0.03, 0.0, 2.0), 0.0625), _metal(rng)))
    scene = _shuffled(rng, _room(rng, lo, hi), others, _orders(seed))
    return scene, _camera(frame=frame, fov=fov), _kw(rng, seed), "fov %.2f on %dx%d" % (fov, frame[0], frame[1])


def irregular(seed, lens=False):
    """shuffled_room plus a Metal sphere of roughness 0: the scene is outside the regular class, so every shortcut is off (no axis pairs, no
    candidate sets, black paths traced on, shade_last_depth) and a sample may be NaN: NaN for NaN."""
    scene, cam, kw, note = shuffled_room(seed + 1)
    rng = np.random.default_rng([12, seed])
    scene.objects.insert(int(rng.integers(0, len(scene.objects) + 1)), Object(Sphere((0.25, -0.25, 2.0), 0.5), Material.Metal((1.0, 0.9, 0.8), 0.0)))
    return scene, cam, kw, note + ", a roughness-0 sphere"


# ---------------------------------------------------------------- the tile classes (primary_candidates.hpp: TILE CLASSES)
# The classes above leave most wave tiles general: over all their cases the host probe finds 15 BLACK and 37 EMITTER tiles.  The ones below are
# rooms looked at so that whole wave tiles see ONE wall, which a work item of the role-sorted kernel then ends as an EMITTER or a BLACK item.
def _plain(rng):
    """a coloured Diffuse or a Metal: a wall that is neither black nor a light"""
    return (_diffuse, _metal)[int(rng.integers(0, 2))](rng)


def _walls_by_role(lo, hi, mats):
    """the six walls, keyed (axis, plus); mats: {(axis, plus): Material}"""
    return {(k, plus): Object(_wall(k, plus, lo[k] if plus else hi[k]), mats[(k, plus)]) for k in range(3) for plus in (True, False)}


def _scene_of(objects):
    scene = Scene()
    scene.objects = list(objects)
    return scene


ONE_WALL_MIXED = ((40, 24), (56, 40), (56, 40), (40, 24), (56, 40), (40, 24))  # the frame per seed; the bounce limit is BOUNCE_LIMITS[seed % 4]


def one_wall_mixed(seed, lens=False):
    """Six axis walls, the camera near one side wall: that wall emits and fills the frame's columns on its side, the back wall is black Diffuse and
    fills the others, and the seam between them (and, in the corners, the floor's and the ceiling's) crosses the tiles in between, which stay
    general.  EMITTER, BLACK and GENERAL items in one launch, at every bounce limit (BOUNCE_LIMITS[seed % 4]: a BLACK item at limit 1 parks every
    survivor and ends it); odd seeds put one small sphere in front of the back wall.  The thin-lens variant switches every class off."""
    rng = np.random.default_rng([13, seed])
    frame = ONE_WALL_MIXED[seed % len(ONE_WALL_MIXED)]
    lo = [-_dyadic(rng, 1.5, 2.5), -_dyadic(rng, 2.0, 2.5), -_dyadic(rng, 0.5, 1.5)]
    hi = [_dyadic(rng, 1.5, 2.5), _dyadic(rng, 2.0, 2.5), _dyadic(rng, 3.0, 4.0)]
    right = frame == (40, 24) and seed != 3  # the side wall the camera is near (on the wide frame the left one: the rect lists of the GPU test end at x = 37)
    side = (0, not right)  # (the wall at hi[0] has the normal -e_x)
    mats = {(k, plus): _plain(rng) for k in range(3) for plus in (True, False)}
    mats[side], mats[(2, False)] = _emission(rng), _black(rng)
    near = _dyadic(rng, 0.625, 1.0)
    pos = (hi[0] - near if right else lo[0] + near, _dyadic(rng, -0.25, 0.25), 0.0)
    walls = _walls_by_role(lo, hi, mats)
    others = [Object(Sphere((pos[0] + (-1.0 if right else 1.0), -0.75, 2.5), 0.125), _material(rng))] if seed % 2 else []
    objs = list(walls.values()) + others
    scene = _scene_of(objs[i] for i in rng.permutation(len(objs)))
    fov = (35.0, 55.0)[frame == (56, 40)]
    kw = _kw(rng, seed, lens, bounce_limit=BOUNCE_LIMITS[seed % 4])
    return scene, _camera(pos, frame=frame, fov=fov, lens=lens), kw, "camera %.3f from the emitting %s wall, back wall black, fov %g" % (near, "right" if right else "left", fov)


# one colour per seed: signed zeros, a negative component, the smallest denormal, the smallest normal, the regular class's bound, three ordinary values
EMITTER_COLOURS = ((0.0, -0.0, 1.0), (0.75, -0.5, 1.25), (5e-324, 1.0, -5e-324), (2.0**-1022, 0.5, -(2.0**-1022)), (1e150, 5e-324, -1e150), (0.3, 1.7, 0.9))


def emitter_colours(seed, lens=False):
    """A narrow view of the emitting back wall: every wave tile is an EMITTER item, whose samples are the wall's colour stored as it stands in the
    table — EMITTER_COLOURS[seed].  1e150 is the regular class's bound: 1.0 * x = x, the sum of 160 of them and the moments' 1e300 stay finite, a
    denormal's square underflows to 0; -0.0 must add as the reference's -0.0 does."""
    rng = np.random.default_rng([14, seed])
    colour = EMITTER_COLOURS[seed % len(EMITTER_COLOURS)]
    lo, hi = _bounds(rng)
    mats = {(k, plus): _material(rng) for k in range(3) for plus in (True, False)}
    mats[(2, False)] = Material.Emission(colour)
    objs = list(_walls_by_role(lo, hi, mats).values())
    scene = _scene_of(objs[i] for i in rng.permutation(len(objs)))
    fov = float(rng.uniform(12.0, 20.0))
    pos = (_dyadic(rng, -0.25, 0.25), _dyadic(rng, -0.25, 0.25), 0.0)
    return scene, _camera(pos, fov=fov), _kw(rng, seed, bounce_limit=BOUNCE_LIMITS[seed % 4]), "the back wall emits %r, fov %.1f" % (colour, fov)


# (what, the black wall's colour, its roughness, its place in the table, the bounce limit)
BLACK_WALLS = (("signed zeros", (-0.0, 0.0, -0.0), 0.375, "first", 2), ("roughness 512", (0.0, 0.0, 0.0), 512.0, "last", 5),
               ("roughness 1e-12", (0.0, 0.0, 0.0), 1e-12, "any", 16), ("a black Metal wall beside it", (0.0, 0.0, 0.0), 0.25, "any", 2),
               ("roughness -512", (0.0, -0.0, 0.0), -512.0, "any", 5))


def black_metal_wall(scene):
    """index of the black Metal wall of a scene, or None"""
    return next((i for i, o in enumerate(scene.objects) if o.material.kind == abi.RMD_MAT_METAL and tuple(o.material.color) == (0.0, 0.0, 0.0)), None)


def black_walls(seed, lens=False):
    """A narrow view of the black Diffuse back wall: every wave tile is a BLACK item, every generation trip of the launch a round.  BLACK_WALLS[seed]:
    the colour as signed zeros (kObjBlackDiffuse is set by == 0.0), the roughness the survivors' GGX hits take (512, 1e-12, -512), the wall first
    and last in the table.  Seed 3 looks wider from near the left wall, which is black METAL: prob_d = 0, every sample of it is a specular bounce
    whose Fresnel term (1 - cos)^5 is not zero, and its tiles must stay general.  The ceiling and the wall behind the camera emit, so survivors carry
    light from their second vertex on (no frame is black: a BLACK item at bounce limit 1 is one_wall_mixed's); at roughness 1e-12 that light is
    too faint to show in a sum, and one tile holds a small emitting sphere."""
    rng = np.random.default_rng([15, seed])
    what, colour, rough, place, bounces = BLACK_WALLS[seed % len(BLACK_WALLS)]
    lo, hi = _bounds(rng)
    mats = {(k, plus): _plain(rng) for k in range(3) for plus in (True, False)}
    mats[(2, False)] = Material.Diffuse(colour, rough)
    mats[(1, False)], mats[(2, True)] = _emission(rng), _emission(rng)
    metal = "Metal" in what
    pos, fov = (_dyadic(rng, -0.25, 0.25), _dyadic(rng, -0.25, 0.25), 0.0), float(rng.uniform(12.0, 20.0))
    if metal:
        mats[(0, True)] = Material.Metal((0.0, 0.0, 0.0), 0.875)  # (rough: its lobe reaches the emitting ceiling at the second vertex)
        pos, fov = (lo[0] + 0.75, pos[1], 0.0), 35.0
    walls = _walls_by_role(lo, hi, mats)
    back = walls.pop((2, False))
    rest = list(walls.values())
    if rough == 1e-12:  # what such a mirror returns is 1e-15 a sample: a small light in the middle of ONE tile (28, 4) or (28, 20), which is then general
        ey = math.tan(math.radians(fov) / 2.0)
        rest.append(Object(Sphere((pos[0] + 2.0 * 0.4 * ey * FRAME[0] / FRAME[1], pos[1] + 2.0 * (2.0 / 3.0) * ey, 2.0), 0.03125), _emission(rng)))
    rest = [rest[i] for i in rng.permutation(len(rest))]
    at = {"first": 0, "last": len(rest)}.get(place, int(rng.integers(1, len(rest))))
    scene = _scene_of(rest[:at] + [back] + rest[at:])
    return scene, _camera(pos, fov=fov), _kw(rng, seed, bounce_limit=bounces), "the back wall black Diffuse at %d of the table: %s" % (at, what)


CLASS_TABLE_EDGE = (63, 64, 65)  # objects


def class_table_edge(seed, lens=False):
    """63, 64 and 65 objects (CLASS_TABLE_EDGE[seed]): the six walls first, then small spheres in a lattice in one corner of the view, which the
    other tiles' cones clear, and LAST one small sphere apart from them in front of the black back wall.  With 63 and 64 objects that sphere has a
    bit in the visit mask, its tile is general and the tiles that clear every sphere are classed; with 65 it is object 64, which no mask reaches,
    and NO tile may be classed (primary_one_wall: n_objects - 1 < 64) — a rule that looked at the mask alone would class the tile it sits in."""
    rng = np.random.default_rng([16, seed])
    n = CLASS_TABLE_EDGE[seed % len(CLASS_TABLE_EDGE)]
    lo, hi = [-1.25, -0.875, -1.0], [2.5, 2.0, 3.5]  # (0.8 lo at z = 1.5: the frame's lower left corner at fov 55)
    mats = {(k, plus): _plain(rng) for k in range(3) for plus in (True, False)}
    mats[(2, False)], mats[(1, False)], mats[(1, True)] = _black(rng), _emission(rng), _emission(rng)
    objs = list(_walls_by_role(lo, hi, mats).values())
    objs = [objs[i] for i in rng.permutation(6)]
    for s in range(n - 7):
        i, j = s % 8, s // 8
        objs.append(Object(Sphere((0.8 * lo[0] + 0.02 * i, 0.8 * lo[1] + 0.02 * j, 1.5), 0.03), _material(rng)))
    objs.append(Object(Sphere((0.5, 0.25, 2.5), 0.125), _emission(rng)))  # apart from the others, and the table's last object
    assert len(objs) == n
    return _scene_of(objs), _camera(frame=(56, 40)), _kw(rng, seed, bounce_limit=(5, 2, 5)[seed % 3]), "%d objects, the last a sphere apart from the cluster" % n


# (frame, fov, what the back wall is, the bounce limit)
RAGGED_ONE_WALL = (((1, 1), 12.0, "black", 2), ((1, 8), 12.0, "emitter", 2), ((9, 9), 12.0, "black", 2), ((41, 25), 35.0, "emitter", 5),
                   ((7, 33), 20.0, "black", 16), ((33, 7), 12.0, "black", 2), ((9, 9), 12.0, "emitter", 5))


def ragged_one_wall(seed, lens=False):
    """Frames of 1x1, 1x8, 9x9, 41x25, 7x33 and 33x7 pixels (RAGGED_ONE_WALL[seed]) that look at the back wall alone, black Diffuse or emitting:
    classed wave tiles one pixel wide and one pixel high, a generation round over a single pixel's samples.  The tiny frames at fov 12."""
    rng = np.random.default_rng([17, seed])
    frame, fov, what, bounces = RAGGED_ONE_WALL[seed % len(RAGGED_ONE_WALL)]
    lo, hi = _bounds(rng)
    mats = {(k, plus): _plain(rng) for k in range(3) for plus in (True, False)}
    mats[(1, False)], mats[(2, True)] = _emission(rng), _emission(rng)  # (the ceiling, and the wall behind the camera: a survivor's second vertex)
    mats[(2, False)] = _black(rng) if what == "black" else _emission(rng)
    objs = list(_walls_by_role(lo, hi, mats).values())
    scene = _scene_of(objs[i] for i in rng.permutation(len(objs)))
    pos = (_dyadic(rng, -0.25, 0.25), _dyadic(rng, -0.25, 0.25), 0.0)
    return scene, _camera(pos, frame=frame, fov=fov), _kw(rng, seed, bounce_limit=bounces), "%dx%d at fov %g, the back wall %s" % (frame[0], frame[1], fov, what)


TILE_CLASS_CLASSES = ("one_wall_mixed", "emitter_colours", "black_walls", "class_table_edge", "ragged_one_wall")
CLASSES = {f.__name__: f for f in (shuffled_room, signed_zero_normals, partial_room, duplicate_walls, tilted_pairs, camera_on_walls, coincident_spheres,
                                   table_edges, one_lobe, rough_extremes, fov_and_aspect, irregular, one_wall_mixed, emitter_colours, black_walls,
                                   class_table_edge, ragged_one_wall)}
SEEDS = {"shuffled_room": (0, 1, 2), "signed_zero_normals": (0, 1), "partial_room": (0, 1, 2, 3), "duplicate_walls": (0, 1), "tilted_pairs": (0, 1, 2),
         "camera_on_walls": tuple(range(len(CAMERA_ON_WALLS))), "coincident_spheres": (0, 1), "table_edges": tuple(range(len(TABLE_EDGES))),
         "one_lobe": (0, 1, 2, 3), "rough_extremes": (0, 1), "fov_and_aspect": tuple(range(len(FOV_AND_ASPECT))), "irregular": (0, 1),
         "one_wall_mixed": tuple(range(len(ONE_WALL_MIXED))), "emitter_colours": tuple(range(len(EMITTER_COLOURS))),
         "black_walls": tuple(range(len(BLACK_WALLS))), "class_table_edge": tuple(range(len(CLASS_TABLE_EDGE))),
         "ragged_one_wall": tuple(range(len(RAGGED_ONE_WALL)))}
LENS_CLASSES = ("shuffled_room", "partial_room", "camera_on_walls", "coincident_spheres", "one_wall_mixed")
LENS_SEEDS = (0, 1)  # the seeds whose thin-lens variant is yielded


def cases(classes=None, lens=None):
    """[(class, seed, lens)] — every class and seed, and the thin-lens variants; lens=False / True keeps one kind"""
    out = []
    for name in classes or CLASSES:
        out += [(name, s, False) for s in SEEDS[name]]
        if name in LENS_CLASSES:
            out += [(name, s, True) for s in LENS_SEEDS]
    return [c for c in out if lens is None or c[2] == lens]


def case_id(case):
    return "%s-%d%s" % (case[0], case[1], "-lens" if case[2] else "")


def build(case):
    """-> (Scene, CameraSettings, Settings, note)"""
    name, seed, lens = case
    scene, cam, kw, note = CLASSES[name](seed, lens=lens)
    return scene, cam, Settings(cam, **kw), note


# ---------------------------------------------------------------- what a scene's table must come out as (a reading of the rule, not of the code)
def is_regular(scene):
    for o in scene.objects:
        g, m = o.geometry, o.material
        vals = list(g.origin) + list(m.color) + (list(g.normal) if isinstance(g, Plane) else [g.radius])
        emission = m.kind == abi.RMD_MAT_EMISSION
        if not emission:
            vals.append(m.roughness)
        if not all(abs(v) <= 1e150 for v in vals):  # (false for a NaN)
            return False
        if (isinstance(g, Sphere) and g.radius == 0.0) or (not emission and m.roughness == 0.0):
            return False
    return True


def expected_axis_pairs(scene):
    """The 10-bit fields a scene's launch must carry, from the rule as include/ and DESIGN.md state it: a plane pairs with the FIRST earlier, still
    unpaired plane whose normal is its exact negation; going through the later planes in index order, a pair whose normals are exactly +-e_k
    becomes axis k's pair if that axis has none yet and the later plane's index + 1 fits ten bits (index <= 1022); only in a regular scene.
    -> [field of x, of y, of z] (0 = none, else the later plane's index + 1)"""
    fields = [0, 0, 0]
    if not is_regular(scene):
        return fields
    objs = scene.objects
    partner = {}
    for j, oj in enumerate(objs):
        if not isinstance(oj.geometry, Plane):
            continue
        for i in range(j):
            gi = objs[i].geometry
            if isinstance(gi, Plane) and i not in partner and all(a == -b for a, b in zip(oj.geometry.normal, gi.normal)):
                partner[i], partner[j] = j, i
                break
    for j in sorted(j for j, i in partner.items() if i < j):
        n = objs[j].geometry.normal
        axes = [k for k in range(3) if n[k] != 0.0]
        if len(axes) == 1 and abs(n[axes[0]]) == 1.0 and fields[axes[0]] == 0 and j <= 1022:
            fields[axes[0]] = j + 1
    return fields
