"""The C++ oracle's mesh geometry against a SECOND, independent reading of the reference's source (tests/second_reading.py: plain Python floats,
written from core/src/geometry/{acc_grid.rs:89-185, primitives/triangle.rs:11-68, primitives/aabb.rs:10-31} without looking at
oracle/oracle.cpp) — bit for bit, on the reference's own mesh assets (committed as arrays) and on the procedural stand-in.  The reference has no
tests and its dragon mesh is absent from the checkout; nothing it holds pins the grid walk, so the walk's parity rests on the restatement being a
faithful reading.  Two readings that agree on every ray — hit or miss, distance, triangle index; grazing rays, rays along the axes, rays that start
inside, behind and beyond the box (Q6), zero and negative-zero direction components (Q8), the res.z index quirk (Q5: three of these grids have
res.z != res.y) — are the evidence available."""
import ctypes as C
import os

import numpy as np
import pytest

import second_reading as sr
from raymond_amd import scenes
from raymond_amd.scene import Mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def reference_mesh(name):
    z = np.load(os.path.join(GOLD, "ref_mesh_%s.npz" % name))
    m = Mesh(z["tri_pos"], z["tri_nrm"])
    m.bake_transform((0.0, -0.3, 2.9))  # cli_old/src/main.rs:61
    return m


def rays_for(grid, rng, n):
    lo, hi = np.asarray(grid.bbox_min), np.asarray(grid.bbox_max)
    centre, size = (lo + hi) / 2, hi - lo
    o = centre + rng.uniform(-2.5, 2.5, (n, 3)) * size
    tgt = centre + rng.uniform(-0.6, 0.6, (n, 3)) * size
    d = tgt - o
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    rays = np.concatenate([o, d], axis=1)
    k = n // 16
    rays[0 * k : 1 * k, 3:] = [0.0, 0.0, 1.0]                       # along +z: two zero components (t_delta = inf)
    rays[1 * k : 2 * k, 3:] = [-0.0, -1.0, 0.0]                     # a negative zero: signum(-0.0) = -1
    rays[2 * k : 3 * k, :3] = centre + rng.uniform(-0.45, 0.45, (k, 3)) * size  # origins inside the box
    rays[3 * k : 4 * k, :3] = hi + rng.uniform(0.01, 0.5, (k, 3)) * size        # origins beyond the max corner (Q6: not re-based)
    rays[4 * k : 5 * k, 3] = 0.0                                    # one zero component
    rays[5 * k : 6 * k, 3:] *= -1.0                                 # pointing away from the box
    return rays


@pytest.mark.parametrize("name", ["suzanne_flat", "monkeysmooth", "ico_sphere", "cube", "lumpy"])
def test_oracle_grid_walk_equals_a_second_reading_of_the_source(oracle, name):
    mesh = scenes.lumpy_sphere_mesh(7) if name == "lumpy" else reference_mesh(name)
    if name == "lumpy":
        mesh.bake_transform((0.0, -0.3, 2.9))
    rc, grid = oracle.grid_build(mesh)
    assert rc == 0
    sc = scenes.mesh_scene(Mesh(mesh.tri_pos, mesh.tri_nrm), translate=(0.0, 0.0, 0.0), grid_builder=lambda m: grid)
    osc = oracle.OracleScene(sc)
    rng = np.random.default_rng(len(name))
    n = 1600 if len(mesh) > 500 else 3200
    rays = rays_for(grid, rng, n)
    oh, ot, otri = osc.grid_intersect(0, rays)
    g = {"bbox_min": tuple(map(float, grid.bbox_min)), "bbox_max": tuple(map(float, grid.bbox_max)), "cell_size": tuple(map(float, grid.cell_size)),
         "resolution": tuple(int(v) for v in grid.resolution), "cells": grid.cells.tolist(), "mapping_table": grid.mapping_table.tolist(),
         "tri_pos": [tuple(map(float, p)) for p in grid.tri_pos]}
    assert g["resolution"][2] != g["resolution"][1] or name in ("cube", "ico_sphere")  # (Q5 matters on the other grids)
    hits = 0
    for i in range(n):
        r = sr.grid_intersects(g, tuple(map(float, rays[i, :3])), tuple(map(float, rays[i, 3:])))
        if r is None:
            assert oh[i] == 0, "ray %d: the oracle hits, the second reading misses" % i
        else:
            hits += 1
            assert oh[i] == 1 and otri[i] == r[1], "ray %d: triangle %s vs %s" % (i, otri[i], r[1])
            assert np.float64(ot[i]).tobytes() == np.float64(r[0]).tobytes(), "ray %d: distance %r vs %r" % (i, ot[i], r[0])
    assert 0.1 * n < hits < 0.9 * n  # both outcomes are well represented


def test_oracle_triangle_functions_equal_a_second_reading_of_the_source(oracle):
    """Triangle::intersects, Triangle::get_surface_properties (the Heron-formula normal, incl. hit points ON an edge and a triangle whose
    vertex normals cancel: NaN in both readings) and AABB::intersects, bit for bit."""
    L = oracle.load()
    rng = np.random.default_rng(99)
    n = 4000
    pos = rng.uniform(-1, 1, (n, 9))
    nrm = rng.normal(size=(n, 9))
    for k in range(3):
        nrm[:, 3 * k : 3 * k + 3] /= np.sqrt((nrm[:, 3 * k : 3 * k + 3] ** 2).sum(axis=1))[:, None]
    nrm[:50] = 0.0  # vertex normals that sum to zero
    w = rng.dirichlet((1, 1, 1), n)
    w[50:250, 2] = 0.0  # hit points exactly on edge p0p1 (Heron's radicand may round below zero)
    w[50:250] /= w[50:250].sum(axis=1)[:, None]
    target = w[:, :1] * pos[:, 0:3] + w[:, 1:2] * pos[:, 3:6] + w[:, 2:3] * pos[:, 6:9]
    target[2000:] += rng.normal(scale=0.3, size=(n - 2000, 3))  # half of the rays aim beside the triangle
    origin = rng.uniform(-3, 3, (n, 3))
    d = target - origin
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    rays = np.concatenate([origin, d], axis=1)
    hit, t = np.zeros(n, dtype=np.int32), np.zeros(n)
    L.orc_triangle_intersect(n, oracle.ptr(pos), oracle.ptr(rays), oracle.ptr(hit), oracle.ptr(t))
    tt = np.where(hit == 1, t, 1.0)
    on = np.zeros((n, 3))
    L.orc_triangle_normal(n, oracle.ptr(pos), oracle.ptr(nrm), oracle.ptr(rays), oracle.ptr(tt), oracle.ptr(on))
    boxes = np.sort(rng.uniform(-1, 1, (n, 2, 3)), axis=1).reshape(n, 6)
    bh, bt = np.zeros(n, dtype=np.int32), np.zeros(n)
    L.orc_aabb_intersect(n, oracle.ptr(boxes), oracle.ptr(rays), oracle.ptr(bh), oracle.ptr(bt))
    nan_normals = 0
    for i in range(n):
        p = tuple(map(float, pos[i]))
        o, dd = tuple(map(float, rays[i, :3])), tuple(map(float, rays[i, 3:]))
        r = sr.triangle_intersects(p[0:3], p[3:6], p[6:9], o, dd)
        assert (r is not None) == bool(hit[i]), i
        if r is not None:
            assert np.float64(r).tobytes() == np.float64(t[i]).tobytes(), i
        nn = sr.triangle_normal((p[0:3], p[3:6], p[6:9]), (tuple(map(float, nrm[i, 0:3])), tuple(map(float, nrm[i, 3:6])), tuple(map(float, nrm[i, 6:9]))), o, dd, float(tt[i]))
        for c in range(3):
            same = np.float64(nn[c]).tobytes() == np.float64(on[i, c]).tobytes() or (nn[c] != nn[c] and on[i, c] != on[i, c])
            assert same, (i, c, nn[c], on[i, c])
        nan_normals += nn[0] != nn[0]
        b = sr.aabb_intersects(tuple(map(float, boxes[i, :3])), tuple(map(float, boxes[i, 3:])), o, dd)
        assert (b is not None) == bool(bh[i]), i
        if b is not None:
            assert np.float64(b).tobytes() == np.float64(bt[i]).tobytes(), i
    assert hit.sum() > 1500 and nan_normals >= 50


# ================================================================ the whole radiance path
def grid_dict(grid):
    return {"bbox_min": tuple(map(float, grid.bbox_min)), "bbox_max": tuple(map(float, grid.bbox_max)), "cell_size": tuple(map(float, grid.cell_size)),
            "resolution": tuple(int(v) for v in grid.resolution), "cells": grid.cells.tolist(), "mapping_table": grid.mapping_table.tolist(),
            "tri_pos": [tuple(map(float, p)) for p in grid.tri_pos], "tri_nrm": [tuple(map(float, p)) for p in grid.tri_nrm]}


def second_reading_scene(scene, cam):
    from raymond_amd import abi
    from raymond_amd.scene import Grid, Plane, Sphere

    kinds = {abi.RMD_MAT_DIFFUSE: "diffuse", abi.RMD_MAT_METAL: "metal", abi.RMD_MAT_EMISSION: "emission"}
    objects, grids = [], {}
    for o in scene.objects:
        g, m = o.geometry, o.material
        d = {"material": (kinds[m.kind], m.color, m.roughness)}
        if isinstance(g, Plane):
            d.update(kind="plane", origin=g.origin, normal=g.normal)
        elif isinstance(g, Sphere):
            d.update(kind="sphere", origin=g.origin, radius=g.radius)
        else:
            assert isinstance(g, Grid)
            if id(g.grid) not in grids:
                grids[id(g.grid)] = grid_dict(g.grid)
            d.update(kind="grid", grid=grids[id(g.grid)])
        objects.append(d)
    c = {"width": cam.backbuffer_width, "height": cam.backbuffer_height, "fov_vert": cam.fov_vert, "position": cam.transform.position,
         "focal_length": cam.focal_length, "aperture_radius": cam.aperture_radius}
    return {"objects": objects, "camera_position": cam.transform.position}, c


def same_f64(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (a != a and b != b)


def hold_oracle_to_second_reading(oracle, scene, settings, pixels, samples_per_pixel, want_depths, want_object=0, min_nonzero=None, vertices_every=97):
    """min_nonzero: how many samples must carry radiance (default: more than a twentieth; -1 for a scene that is black by construction);
    vertices_every: the vertex sequences are compared on every so-manyth sample (1: on all of them)."""
    cam = settings.camera_settings
    osc = oracle.OracleScene(scene)
    sc, c = second_reading_scene(scene, cam)
    st = {"bounce_limit": settings.bounce_limit}
    xy = np.repeat(np.asarray(pixels, dtype=np.uint32), samples_per_pixel, axis=0)
    smp = np.tile(np.arange(samples_per_pixel, dtype=np.uint32), len(pixels))
    got = osc.trace_samples(cam, settings, xy, smp)
    depths, nonzero, through_object = {}, 0, 0
    for i in range(len(smp)):
        path = []
        rgb = sr.sample_pixel(sc, c, st, settings.seed, int(xy[i, 0]), int(xy[i, 1]), int(smp[i]), use_dof=settings.use_dof, path=path)
        for ch in range(3):
            assert same_f64(rgb[ch], got[i, ch]), "pixel %s sample %d channel %d: %r (second reading) vs %r (oracle); path %s" % (
                tuple(xy[i]), smp[i], ch, rgb[ch], got[i, ch], path)
        depths[len(path)] = depths.get(len(path), 0) + 1
        nonzero += any(v != 0.0 for v in rgb)
        through_object += any(o == want_object for o, _ in path)
        if i % vertices_every == 0:  # the vertices as well, on a subset
            _, po, ps = osc.trace_sample_path(cam, settings, int(xy[i, 0]), int(xy[i, 1]), int(smp[i]))
            assert [p[0] for p in path] == po.tolist()[: len(path)], (i, path, po)
    assert nonzero > (len(smp) // 20 if min_nonzero is None else min_nonzero) and through_object > len(smp) // 20
    for d in want_depths:
        assert depths.get(d, 0) > 0, depths
    return depths


def test_oracle_radiance_equals_a_second_reading_of_trace_on_the_spheres_scene(oracle):
    """trace() (src/trace.rs:232-320), Scene::intersect, Sphere / Plane, the BRDF helpers and the two samplers, bit for bit over every sample of
    a pixel lattice: both lobes on both spheres, the emissive ceiling, the black walls, paths cut at the bounce limit."""
    scene = scenes.reflective_spheres()
    settings = scenes.config_settings("C1", spp=6)
    settings.bounce_limit = 5
    w, h = settings.camera_settings.backbuffer_width, settings.camera_settings.backbuffer_height
    pixels = [(x, y) for y in range(3, h, 5) for x in range(2, w, 5)]
    hold_oracle_to_second_reading(oracle, scene, settings, pixels, 6, want_depths=(1, 2, 3, 4, 5))


@pytest.mark.parametrize("name,use_dof", [("lumpy", False), ("lumpy", True), ("suzanne_flat", False), ("monkeysmooth", False)])
def test_oracle_radiance_equals_a_second_reading_of_trace_on_a_mesh_scene(oracle, name, use_dof):
    """The same with a mesh behind an AccGrid in the scene (grid walk, Moller-Trumbore, the Heron normal) and, opted in, the thin lens
    (generate_primary_ray_with_dof, :335-360: rejection loop, focal plane)."""
    if name == "lumpy":
        mesh = scenes.lumpy_sphere_mesh(21)
    else:
        z = np.load(os.path.join(GOLD, "ref_mesh_%s.npz" % name))
        mesh = Mesh(z["tri_pos"], z["tri_nrm"])
    scene = scenes.mesh_scene(mesh, grid_builder=lambda m: oracle.grid_build(m)[1])
    cam = scenes.camera(160, 90, aperture_radius=0.5 if use_dof else 0.0)
    from raymond_amd.scene import Settings

    settings = Settings(cam, sample_count=4, bounce_limit=5, seed=scenes.SEED + 7, use_dof=use_dof)
    pixels = [(x, y) for y in range(1, 90, 3) for x in range(2, 160, 3)]
    depths = hold_oracle_to_second_reading(oracle, scene, settings, pixels, 4, want_depths=(1, 2, 3), want_object=1)
    assert sum(depths.values()) == len(pixels) * 4


def test_second_reading_philox_known_answers():
    """Random123's known-answer vectors for philox4x32-10 (kat_vectors), on the plain-Python restatement."""
    assert sr.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert sr.philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert sr.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_oracle_output_stage_equals_a_second_reading_of_the_source(oracle):
    """cli_old/src/main.rs:161-181 (tone map, gamma, the Vector3 cast to u8 that fails as a whole) byte for byte, incl. negative, huge, infinite and NaN sums."""
    rng = np.random.default_rng(5)
    n = 6000
    acc = rng.exponential(40.0, (n, 3))
    acc[:200] *= 1e-6
    acc[200:400] *= 1e3
    acc[400:420, 1] = np.nan
    acc[420:440, 0] = np.inf
    acc[440:460, 2] = -np.inf
    acc[460:520] *= -1.0  # negative radiance: 1 - exp(+x) < 0, powf of a negative base is NaN -> the whole pixel stays black
    acc[520:540] = 0.0
    acc[540:560, 0] = -1e-300
    spp = 64
    got = oracle.resolve_tonemap(acc, spp)
    for i in range(n):
        want = sr.resolve_pixel(tuple(map(float, acc[i])), float(spp))
        assert tuple(int(v) for v in got[i]) == want, (i, acc[i], got[i], want)
    assert (got > 0).any(axis=1).mean() > 0.8 and (got[400:420] == 0).all() and (got[440:520] == 0).all() and (got[420:440, 0] == 255).all()
