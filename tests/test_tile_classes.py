"""The tile classes of the spheres kernel's work items (raymond_amd/csrc/primary_candidates.hpp: TILE CLASSES), held to the oracle on the CPU.

A work item whose 8x8 wave tile sees ONE wall — whatever the jitter — is an EMITTER item when that wall emits (every sample is the wall's colour;
the kernel draws no random number and makes no ray for it) or a BLACK item when it is black and diffuse (a sample whose block 0 has
lobe_bits < 2^21 is (0, 0, 0); the kernel makes rays for the others only).  The host-only probe rmd_probe_tile_classes evaluates the very
functions the kernel calls; for every tile it does not call general this test asserts
  * every primary ray the oracle makes for the tile — orc_primary_ray at the jitter extremes u = 0 and u = 1 - 2^-53 and orc_sample_primary_rays'
    own jitters, at the four corner pixels and, for every tenth tile, at all of its pixels — hits the predicted object under the oracle's
    Scene::intersect,
  * EMITTER: the oracle's sample is the wall's colour, bit for bit; BLACK: the oracle's sample with lobe_bits < 2^21 is (0, 0, 0),
over a few hundred seeded rooms (0 .. 64 spheres, walls at non-unit distances, emitters on any wall, black Metal walls — prob_d = 0, which must be
general) and cameras (anywhere inside, next to a wall, next to two walls: looking along one).  At least 30 % of the campaign's tiles are not
general, so the test cannot pass by never classing anything."""
import numpy as np
import pytest

from raymond_amd import probe, scenes
from raymond_amd.scene import CameraSettings, Material, Object, Plane, Scene, Settings, Sphere, Transform
from test_primary_candidates import ONE_MINUS, tile_rays, wave_tiles

SEED = 0x7117E
N_CASES = 300
N_SAMPLED = 12  # (pixel, sample) pairs per tile whose rays and samples come from the oracle's own RNG

WALL_MATERIALS = (
    ("emitter", lambda rng: Material.Emission(tuple(float(v) for v in rng.uniform(0.2, 3.0, 3)))),
    ("black", lambda rng: Material.Diffuse((0.0, 0.0, 0.0), float(rng.uniform(0.05, 0.9)))),
    ("grey", lambda rng: Material.Diffuse((0.7, 0.6, 0.5), 0.5)),
    ("black_metal", lambda rng: Material.Metal((0.0, 0.0, 0.0), 0.2)),  # prob_d = 0, not 0.5: general
    ("metal", lambda rng: Material.Metal((0.9, 0.8, 0.1), 0.1)),
)


def random_room(rng, n_spheres):
    """An axis-aligned room of six walls at non-unit distances, the walls' materials drawn per wall, the spheres anywhere inside."""
    lo, hi = -rng.uniform(0.4, 7.0, 3), rng.uniform(0.4, 7.0, 3)
    objs, kinds = [], []
    for k in range(3):
        e, o_lo, o_hi = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        e[k], o_lo[k], o_hi[k] = 1.0, lo[k], hi[k]
        for origin, normal in ((o_lo, e), (o_hi, [-v for v in e])):
            name, make = WALL_MATERIALS[int(rng.choice(5, p=[0.35, 0.45, 0.08, 0.06, 0.06]))]
            objs.append(Object(Plane(origin, normal), make(rng)))
            kinds.append(name)
    sphere_mats = [Material.Diffuse((0.7, 0.7, 0.7), 0.5), Material.Emission((1.5, 1.5, 1.5)), Material.Diffuse((0.0, 0.0, 0.0), 0.3), Material.Metal((0.9, 0.8, 0.1), 0.1)]
    for _ in range(n_spheres):
        c = rng.uniform(lo, hi)
        objs.append(Object(Sphere(c, float(rng.choice([0.02, 0.1, 0.3, 0.8]) * rng.uniform(0.5, 1.5))), sphere_mats[int(rng.integers(0, 4))]))
        kinds.append("sphere")
    order = rng.permutation(len(objs))
    scene = Scene()
    scene.objects = [objs[i] for i in order]
    return scene, [kinds[i] for i in order], lo, hi


def random_camera(rng, lo, hi, case):
    W, H = int(rng.integers(17, 161)), int(rng.integers(17, 161))
    fov = float(rng.choice([12.0, 35.0, 55.0, 90.0, 120.0]) * rng.uniform(0.9, 1.1))
    pos = rng.uniform(lo * 0.9, hi * 0.9)
    kind = case % 4
    if kind in (1, 2):  # next to a wall: a little inside it, or a hair (1e-10: ON the wall by make_params' rule — black bounces are traced on and every tile is general)
        k = int(rng.integers(0, 3))
        pos[k] = (lo[k], hi[k])[int(rng.integers(0, 2))] * (1.0 - float(rng.choice([1e-10, 1e-6, 1e-6, 1e-3, 1e-3, 1e-2])))
    if kind == 2:  # ... and next to a side wall as well: the rays run along it
        k = int(rng.integers(0, 2))
        pos[k] = (lo[k], hi[k])[int(rng.integers(0, 2))] * (1.0 - float(rng.choice([1e-7, 1e-4])))
    return CameraSettings(W, H, fov, Transform(tuple(float(v) for v in pos)))


def tile_pixels(tile, every_pixel):
    x0, y0, w, h = (int(v) for v in tile)
    if every_pixel:
        return [(x, y) for y in range(y0, y0 + h) for x in range(x0, x0 + w)]
    return sorted({(x0, y0), (x0 + w - 1, y0), (x0, y0 + h - 1), (x0 + w - 1, y0 + h - 1)})


def extreme_rays(oracle, cam, pixels):
    """orc_primary_ray at the four jitter corners (0 and 1 - 2^-53 in x and in y) of every pixel given"""
    import ctypes as C

    xy = np.array([p for p in pixels for _ in range(4)], dtype=np.uint32)
    u = np.array([(ux, uy) for _ in pixels for ux in (0.0, ONE_MINUS) for uy in (0.0, ONE_MINUS)])
    rays = np.zeros((xy.shape[0], 6))
    c = cam.pod()
    oracle.load().orc_primary_ray(xy.shape[0], C.byref(c), oracle.ptr(xy), oracle.ptr(u), oracle.ptr(rays))
    return rays


def check_classed_tile(oracle, full, scene, cam, st, tile, cls, wall, rng, stats, every_pixel):
    o = scene.objects[wall]
    assert isinstance(o.geometry, Plane)
    pixels = tile_pixels(tile, every_pixel)
    rays = extreme_rays(oracle, cam, pixels)
    # the oracle's own samples: its jitter for (pixel, sample), the ray it makes of it and the sample it computes
    pick = rng.integers(0, len(pixels), N_SAMPLED)
    xy = np.array([pixels[i] for i in pick], dtype=np.uint32)
    smp = rng.integers(0, 1 << 20, N_SAMPLED).astype(np.uint32)
    own, ok = oracle.sample_primary_rays(cam, st.seed, False, xy, smp)
    assert ok.all()
    obj, _, _ = full.scene_intersect(np.concatenate([rays, own, tile_rays(oracle, cam, tile, rng)]))
    assert (obj == wall).all(), ("a primary ray of a classed tile hits another object", tile, cls, wall, np.unique(obj))
    stats["rays"] += obj.shape[0]
    rgb = full.trace_samples(cam, st, xy, smp)
    if cls == probe.TILE_EMITTER:
        assert o.material.kind == Material.Emission((0, 0, 0)).kind
        colour = np.array(o.material.color, dtype=np.float64)
        assert (rgb.view(np.uint64) == colour.view(np.uint64)[None, :]).all(), ("an emitter tile's sample is not the colour", tile, wall)
        stats["emitter_samples"] += N_SAMPLED
    else:
        assert cls == probe.TILE_BLACK and tuple(o.material.color) == (0.0, 0.0, 0.0) and o.material.kind == Material.Diffuse((0, 0, 0), 1).kind
        W = cam.backbuffer_width
        r22 = oracle.block_uniforms(st.seed, xy[:, 1].astype(np.int64) * W + xy[:, 0], smp, np.zeros(N_SAMPLED, dtype=np.int64))[:, 2]
        low = r22 * 4194304.0 < float(1 << 21)
        # (a zero of either sign: the reference's is weight * 0 and the weight may be negative — added to a pixel's sum the two are the same addition)
        assert (rgb[low] == 0.0).all(), ("a black tile's sample with lobe_bits < 2^21 is not (0, 0, 0)", tile, wall)
        stats["black_zero_samples"] += int(low.sum())
        stats["black_survivors"] += int((~low).sum())


def test_classed_tiles_see_one_wall_and_their_samples_are_what_the_class_says(oracle, product_lib):
    rng = np.random.default_rng(SEED)
    stats = dict(tiles=0, emitter=0, black=0, rays=0, emitter_samples=0, black_zero_samples=0, black_survivors=0, cases_on=0, black_metal_walls_seen=0)
    for case in range(N_CASES):
        n_spheres = int(rng.choice([0, 0, 0, 1, 1, 2, 5, 20, 64]))  # (with 64 spheres the scene has 70 objects: every tile is general)
        scene, kinds, lo, hi = random_room(rng, n_spheres)
        cam = random_camera(rng, lo, hi, case)
        st = Settings(cam, sample_count=1, bounce_limit=int(rng.integers(1, 6)), seed=int(rng.integers(1, 1 << 62)))
        tiles = wave_tiles(cam.backbuffer_width, cam.backbuffer_height)
        if len(tiles) > 24:
            tiles = tiles[rng.choice(len(tiles), 24, replace=False)]
        on, cls, wall = probe.tile_classes(cam, st, scene, tiles)
        stats["cases_on"] += on
        stats["tiles"] += len(tiles)
        if not on:
            assert (cls == probe.TILE_GENERAL).all() and (wall == -1).all()
            continue
        full = oracle.OracleScene(scene)
        for i, (tile, c, w) in enumerate(zip(tiles, cls, wall)):
            if c == probe.TILE_GENERAL:
                assert w == -1
                continue
            assert 0 <= w < len(scene.objects)
            # the class follows the wall's record: an emitter, or black AND diffuse (prob_d = 0.5); a black Metal wall (prob_d = 0) is never classed
            assert kinds[w] == ("emitter" if c == probe.TILE_EMITTER else "black"), (kinds[w], c)
            stats["emitter" if c == probe.TILE_EMITTER else "black"] += 1
            check_classed_tile(oracle, full, scene, cam, st, tile, int(c), int(w), rng, stats, every_pixel=(stats["emitter"] + stats["black"]) % 10 == 0)
        stats["black_metal_walls_seen"] += kinds.count("black_metal")
    print(stats)
    share = (stats["emitter"] + stats["black"]) / stats["tiles"]
    print("tiles that are not general: %.1f %%" % (100 * share))
    assert share >= 0.30, stats
    assert stats["emitter"] > 500 and stats["black"] > 500 and stats["black_zero_samples"] > 2000 and stats["black_survivors"] > 2000, stats
    assert stats["black_metal_walls_seen"] > 30 and stats["cases_on"] > 0.8 * N_CASES, stats


def test_every_tile_is_general_outside_the_conditions(product_lib):
    sc = scenes.reflective_spheres()
    W, H = 256, 144
    tiles = wave_tiles(W, H)
    cam = scenes.camera(W, H)
    st = Settings(cam, sample_count=1)
    on, cls, wall = probe.tile_classes(cam, st, sc, tiles)
    assert on and (cls == probe.TILE_EMITTER).any() and (cls == probe.TILE_BLACK).any()

    def general(cam, st, scene, tunable=0):
        on, cls, wall = probe.tile_classes(cam, st, scene, tiles, tunable)
        assert not on and (cls == probe.TILE_GENERAL).all() and (wall == -1).all()

    for tunable in (1, 2, 3):  # the switch: 3 = the candidate sets without the classes
        general(cam, st, sc, tunable)
    # ... and 3 leaves the candidate sets as 0 has them
    assert all(np.array_equal(a, b) for a, b in zip(probe.primary_candidates(cam, st, sc, tiles, 3)[2:], probe.primary_candidates(cam, st, sc, tiles, 0)[2:]))
    general(cam, Settings(cam, sample_count=1, trace_black_paths=True), sc)  # black bounces are traced on: no black tile (and no class at all)
    cam_dof = scenes.camera(W, H, aperture_radius=0.05)
    general(cam_dof, Settings(cam_dof, sample_count=1, use_dof=True), sc)
    irregular = scenes.reflective_spheres()
    irregular.objects.append(Object(Sphere((0.0, 0.0, 3.0), 0.3), Material.Metal((1.0, 1.0, 1.0), 0.0)))
    general(cam, st, irregular)
    for pos in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0)):
        c = CameraSettings(W, H, 55.0, Transform(pos))
        general(c, Settings(c, sample_count=1), sc)
    # a tilted plane has a turn in the object loop: every tile that could see it keeps the general code — here all of them
    tilted = scenes.reflective_spheres()
    tilted.objects.append(Object(Plane((0.0, 0.0, 100.0), (0.0, 0.6, -0.8)), Material.Diffuse((0.5, 0.5, 0.5), 0.5)))
    on, cls, wall = probe.tile_classes(cam, st, tilted, tiles)
    assert on and (cls == probe.TILE_GENERAL).all()


def test_the_benchmark_frame_has_classed_tiles(product_lib):
    sc = scenes.reflective_spheres()
    st = scenes.config_settings("C2")
    cam = st.camera_settings
    tiles = wave_tiles(cam.backbuffer_width, cam.backbuffer_height)
    on, cls, wall = probe.tile_classes(cam, st, sc, tiles)
    emitter, black = float((cls == probe.TILE_EMITTER).mean()), float((cls == probe.TILE_BLACK).mean())
    print("C2: emitter tiles %.2f %%, black tiles %.2f %% of %d" % (100 * emitter, 100 * black, len(tiles)))
    assert on and emitter > 0.02 and black > 0.25


@pytest.mark.parametrize("name", ["C1", "C2"])
def test_benchmark_frames_against_the_oracle(oracle, product_lib, name):
    rng = np.random.default_rng(5)
    sc = scenes.reflective_spheres()
    st = scenes.config_settings(name)
    cam = st.camera_settings
    tiles = wave_tiles(cam.backbuffer_width, cam.backbuffer_height)
    if len(tiles) > 512:
        tiles = tiles[rng.choice(len(tiles), 512, replace=False)]
    on, cls, wall = probe.tile_classes(cam, st, sc, tiles)
    assert on
    full = oracle.OracleScene(sc)
    stats = dict(rays=0, emitter_samples=0, black_zero_samples=0, black_survivors=0)
    n = 0
    for tile, c, w in zip(tiles, cls, wall):
        if c != probe.TILE_GENERAL:
            check_classed_tile(oracle, full, sc, cam, st, tile, int(c), int(w), rng, stats, every_pixel=n % 10 == 0)
            n += 1
    assert n > 0.25 * len(tiles) and stats["black_zero_samples"] > 0, (n, stats)
