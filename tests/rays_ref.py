"""The expected records of rmd_intersect_rays, and the ray sets its tests run — shared by tests/test_rays_host.py and tests/test_gpu_rays.py.

A record is composed from the oracle's entry points and nothing else: OracleScene.scene_intersect gives (object, t, triangle), first_hit_ref.hit_features
the normal rmd_render_features defines there; a miss is {0, {0, 0, 0}, -1, 0} and `triangle` is 0 unless the object is a mesh.  `variant` names one of three
wrong readings, which tests/test_rays_host.py tells from the right one.

The ray sets, each a list of (label, rays) batches on one scene:
  (a) grid_rays.adversarial_rays on the rooms tests/test_gpu_grid_walk.py builds around each builder-made grid and the stand-in — the batches of its
      probe test, class by class and shuffled;
  (b) for every case of sphere_scenes.cases() and mesh_scenes.cases() whose frame is one of the small ones (40 x 24, 44 x 27): the sample-0 primary rays of
      orc_sample_primary_rays, the thin lens included, and from each primary hit one incoherent ray — origin frag + N * 1e-5, direction a seeded draw on
      the whole unit sphere;
  (c) the classes whose grids sit at object positions 63 / 64 / 70 and on both sides of 64, three_grids and nan_normals: (b)'s rays of the case and the
      adversarial rays of each of its grids;
  (d) object tables of 511 / 512 / 1,201 objects (tests/test_gpu_features_scenes.py: table_scene), a 40 x 24 pinhole frame's rays and their incoherent rays.
References are computed once per process, shared and read-only.
"""
import collections
import functools
import zlib

import numpy as np

import first_hit_ref as fr
import grid_rays
import oracle_lib as O
from raymond_amd import render, scenes
from raymond_amd.scene import CameraSettings, Grid, Mesh, Object, Scene, Transform

HIT_DTYPE = render.HIT_DTYPE
MISS = np.zeros(1, dtype=HIT_DTYPE)
MISS["object"] = -1
VARIANTS = ("higher_index_wins_ties", "normal_at_origin", "triangle_kept_off_the_mesh")
SMALL_FRAMES = ((40, 24), (44, 27))
OFFSET = 1e-5  # the incoherent ray starts this far along the normal, as the render's bounce rays do (src/trace.rs:261-269)
K_GRID = 24  # adversarial rays per class and grid in set (c)
TABLES = (511, 512, 1201)  # objects: at and past the 64 KB LDS opt-in, and the largest table a launch holds
ROOMS = ("standin", "suzanne_flat", "monkeysmooth", "ico_sphere", "cube", "lumpy")  # test_gpu_grid_walk's probe test: the stand-in and test_grid_rays_host.BUILT
C_CLASSES = {"grid_positions": (2, 3, 4, 5), "three_grids": None, "nan_normals": None}  # class -> its seeds (None: all)

RaySet = collections.namedtuple("RaySet", "label scene batches tunables")  # batches: [(label, (n, 6) rays)]


def _kinds(scene):
    objs = scene.flatten()[0]
    return np.array([int(objs[i].geometry_kind) for i in range(len(scene.objects))], dtype=np.int64)


def _reversed(scene):
    sc = Scene()
    sc.objects = list(scene.objects[::-1])
    return sc


def expected_records(scene, rays, variant=None, osc=None):
    """-> (n,) HIT_DTYPE records of `rays` on `scene`"""
    assert variant is None or variant in VARIANTS
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    osc = osc or O.OracleScene(scene)
    obj, t, sub = osc.scene_intersect(rays)
    kinds = _kinds(scene)
    on_mesh = (obj >= 0) & (kinds[np.maximum(obj, 0)] == 2)
    assert not sub[~on_mesh].any()  # the oracle's triangle index is 0 off a mesh
    if variant == "higher_index_wins_ties":  # Scene::intersect with `<=`: the scan in reverse order keeps the highest index of the closest distance
        robj, rt, rsub = O.OracleScene(_reversed(scene)).scene_intersect(rays)
        obj = np.where(robj >= 0, len(scene.objects) - 1 - robj, -1).astype(np.int32)
        t, sub = rt, rsub
        on_mesh = (obj >= 0) & (kinds[np.maximum(obj, 0)] == 2)
    at = np.zeros_like(t) if variant == "normal_at_origin" else t  # frag = ro + rd * 0
    normal = fr.hit_features(scene, rays, obj, at, sub)[:, 0:3]
    tri = np.where(on_mesh, sub, 0).astype(np.uint32)
    if variant == "triangle_kept_off_the_mesh":  # a triangle index left from a mesh the ray meets, though another object is the closest hit
        for g in range(int(scene.flatten()[3])):
            gh, _, gtri = osc.grid_intersect(g, rays)
            tri = np.where((obj >= 0) & ~on_mesh & (gh != 0) & (tri == 0), gtri, tri).astype(np.uint32)
    out = np.zeros(len(rays), dtype=HIT_DTYPE)
    hit = obj >= 0
    out["object"] = np.where(hit, obj, -1)
    out["t"] = np.where(hit, t, 0.0)
    out["normal"] = np.where(hit[:, None], normal, 0.0)
    out["triangle"] = np.where(hit, tri, 0)
    return out


def incoherent_rays(rays, rec, seed):
    """one ray per hit of `rec`: origin frag + N * OFFSET, direction uniform on the unit sphere (seeded numpy normals, normalised)"""
    hit = rec["object"] >= 0
    r, h = rays[hit], rec[hit]
    with np.errstate(all="ignore"):
        frag = r[:, 0:3] + r[:, 3:6] * h["t"][:, None]
        origin = frag + h["normal"] * OFFSET
    d = np.random.default_rng([0x1257, seed]).normal(size=(len(r), 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    return np.ascontiguousarray(np.concatenate([origin, d], axis=1))


def _frame_rays(scene, cam, seed, use_dof, salt):
    """the frame's sample-0 primary rays and the incoherent rays off their hits, as one batch, primary rays first"""
    xy, _ = fr.pixel_grid(cam.backbuffer_width, cam.backbuffer_height)
    rays, _ok = O.sample_primary_rays(cam, seed, use_dof, xy, np.zeros(len(xy), dtype=np.uint32))  # (no ray: six zeros, which hit nothing)
    rec = expected_records(scene, rays)
    return np.ascontiguousarray(np.concatenate([rays, incoherent_rays(rays, rec, salt)]))


def _salt(key):
    return zlib.crc32(repr(key).encode())


# ---------------------------------------------------------------- (a)
def room_scene(name):
    """test_gpu_grid_walk.test_scene_intersect_equals_the_oracle_on_adversarial_rays' scene for `name`"""
    import test_grid_rays_host as gh

    if name == "standin":
        return scenes.gold_dragon_standin(n=24)
    mesh = gh.small_mesh(name)  # (baked already)
    grid = gh.small_grid(O, name)
    return scenes.mesh_scene(Mesh(mesh.tri_pos, mesh.tri_nrm), translate=(0.0, 0.0, 0.0), grid_builder=lambda m: grid)


@functools.lru_cache(maxsize=None)
def set_a(name):
    from test_gpu_grid_walk import batches_for

    scene = room_scene(name)
    assert isinstance(scene.objects[1].geometry, Grid)
    return RaySet("a/" + name, scene, _frozen(batches_for(scene.objects[1].geometry.grid, name)), {})


# ---------------------------------------------------------------- (b), (c)
def keys_b():
    out = []
    for key in fr.feature_keys():
        cam = fr.feature_case(key).cam
        if (cam.backbuffer_width, cam.backbuffer_height) in SMALL_FRAMES:
            out.append(key)
    return out


def keys_c():
    return [k for k in fr.feature_keys() if k[0] == "mesh" and k[1] in C_CLASSES and (C_CLASSES[k[1]] is None or k[2] in C_CLASSES[k[1]])]


@functools.lru_cache(maxsize=None)
def set_b(key):
    fc = fr.feature_case(key)
    rays = _frame_rays(fc.scene, fc.cam, fc.seed, fc.use_dof, _salt(key))
    return RaySet("b/" + fr.feature_key_id(key), fc.scene, _frozen([("frame", rays)]), fc.tunables)


@functools.lru_cache(maxsize=None)
def set_c(key):
    import mesh_scenes as ms

    fc = fr.feature_case(key)
    batches = [("frame", set_b(key).batches[0][1])]
    for g, grid in enumerate(ms.distinct_grids(fc.scene)):
        by_class = grid_rays.adversarial_rays(grid, np.random.default_rng([0xC, _salt(key), g]), K_GRID)
        batches.append(("grid %d" % g, np.concatenate([by_class[cls] for cls in grid_rays.CLASSES])))
    return RaySet("c/" + fr.feature_key_id(key), fc.scene, _frozen(batches), fc.tunables)


# ---------------------------------------------------------------- (d)
TABLE_CAMERA = CameraSettings(40, 24, 55.0, Transform((0.0, 0.0, 0.0)))
TABLE_SEED = 0x7AB1E


@functools.lru_cache(maxsize=None)
def set_d(n_objects):
    from test_gpu_features_scenes import table_scene

    scene = table_scene(n_objects)
    return RaySet("d/%d objects" % n_objects, scene, _frozen([("frame", _frame_rays(scene, TABLE_CAMERA, TABLE_SEED, False, n_objects))]), {})


def _frozen(batches):
    out = []
    for label, rays in batches:
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        rays.setflags(write=False)
        out.append((label, rays))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(kind, key):
    """-> (RaySet, [records per batch]) of set `kind` ("a" .. "d") at `key`"""
    rs = {"a": set_a, "b": set_b, "c": set_c, "d": set_d}[kind](key)
    osc = O.OracleScene(rs.scene)
    recs = []
    for _, rays in rs.batches:
        rec = expected_records(rs.scene, rays, osc=osc)
        rec.setflags(write=False)
        recs.append(rec)
    return rs, tuple(recs)


def ulps(a, b):
    from test_gpu_parity import ulp_diff

    return ulp_diff(a, b)
