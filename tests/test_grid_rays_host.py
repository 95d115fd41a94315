"""The adversarial ray classes of tests/grid_rays.py on the CPU: for the five builder-made small grids and the hand-built ones (five with res.z > res.y,
res.x = 1 and res.y = 1 among them, and two with tight cell lists), on every class, the oracle's AccGrid::intersects equals the second reading of the source (tests/second_reading.py) bit for bit —
hit, triangle, distance —, the second reading raises on no ray, and both outcomes stay represented in every class that can hit.  This is what makes
the oracle a reference for these rays before tests/test_gpu_grid_walk.py holds the device's walk to it."""
import numpy as np
import pytest

import grid_rays
import second_reading as sr
from raymond_amd import scenes
from raymond_amd.scene import Grid, Material, Mesh, Object, Scene
from test_second_reading import reference_mesh

K = 160  # rays per class and grid (the second reading is plain Python)
BUILT = ("suzanne_flat", "monkeysmooth", "ico_sphere", "cube", "lumpy")
HAND = tuple("hand_%d_%d_%d" % r for r in grid_rays.HAND_RES) + tuple("tight_%d_%d_%d" % r for r in grid_rays.TIGHT_RES)


def small_mesh(name):
    if name == "lumpy":
        m = scenes.lumpy_sphere_mesh(7)
        m.bake_transform((0.0, -0.3, 2.9))
        return m
    return reference_mesh(name)


def small_grid(oracle, name):
    """-> the AccGrid of one of the small grids: the oracle's build of a mesh, or grid_rays.hand_grid on the ico-sphere"""
    if name.startswith(("hand_", "tight_")):
        return grid_rays.hand_grid(reference_mesh("ico_sphere"), tuple(int(v) for v in name.split("_")[1:]), tight=name.startswith("tight_"))
    rc, grid = oracle.grid_build(small_mesh(name))
    assert rc == 0
    return grid


def grid_only_scene(grid):
    sc = Scene()
    sc.objects.append(Object(Grid(grid), Material.Metal((1.0, 1.0, 0.1), 0.15)))
    return sc


@pytest.mark.parametrize("name", BUILT + HAND)
def test_oracle_equals_the_second_reading_on_every_adversarial_class(oracle, name):
    grid = small_grid(oracle, name)
    if name.startswith("hand_"):
        assert grid.resolution[2] > grid.resolution[1]
    osc = oracle.OracleScene(grid_only_scene(grid))
    g = grid_rays.grid_dict(grid)
    rays = grid_rays.adversarial_rays(grid, np.random.default_rng(1000 + len(name)), K)
    again = grid_rays.adversarial_rays(grid, np.random.default_rng(1000 + len(name)), K)
    shares = {}
    for cls in grid_rays.CLASSES:
        r = rays[cls]
        assert r.tobytes() == again[cls].tobytes(), "%s: the generator is not deterministic" % cls
        if cls != "nonfinite":
            assert np.abs(np.sqrt((r[:, 3:] ** 2).sum(axis=1)) - 1.0).max() < 1e-15 * 4, cls
        oh, ot, otri = osc.grid_intersect(0, r)
        for i in range(K):
            s = sr.grid_intersects(g, tuple(map(float, r[i, :3])), tuple(map(float, r[i, 3:])))  # (raises on no ray: an exception fails the test)
            if s is None:
                assert oh[i] == 0, "%s ray %d: the oracle hits, the second reading misses" % (cls, i)
            else:
                assert oh[i] == 1 and otri[i] == s[1], "%s ray %d: triangle %s vs %s" % (cls, i, otri[i], s[1])
                assert np.float64(ot[i]).tobytes() == np.float64(s[0]).tobytes(), "%s ray %d: distance %r vs %r" % (cls, i, ot[i], s[0])
        shares[cls] = float(oh.mean())
    print(name, " ".join("%s %.2f" % kv for kv in shares.items()))
    for cls in grid_rays.CLASSES:
        if cls not in grid_rays.ALL_MISS:
            assert 0.05 < shares[cls] < 0.95, (name, cls, shares)


def test_hand_grid_follows_its_rule():
    """every triangle is listed in each cell its bounding box overlaps whose Q5 index lies inside the array, ascending, and nowhere else"""
    mesh = reference_mesh("ico_sphere")
    for res in grid_rays.HAND_RES:
        g = grid_rays.hand_grid(mesh, res)
        rx, ry, rz = res
        assert g.cells.size == rx * ry * rz and tuple(g.resolution) == res
        assert g.mapping_table.size == g.cells.size + sum(int(g.mapping_table[c]) for c in g.cells)
        pos = mesh.tri_pos.reshape(-1, 3, 3)
        listed = set()
        for c in range(g.cells.size):
            off = int(g.cells[c])
            ids = g.mapping_table[off + 1 : off + 1 + int(g.mapping_table[off])].tolist()
            assert ids == sorted(set(ids))
            listed.update((c, t) for t in ids)
        want = set()
        dropped = 0
        for t in range(pos.shape[0]):
            for z in range(rz):
                for y in range(ry):
                    for x in range(rx):
                        clo = g.bbox_min + np.array([x, y, z]) * g.cell_size
                        chi = g.bbox_min + np.array([x + 1, y + 1, z + 1]) * g.cell_size
                        if (pos[t].min(axis=0) <= chi).all() and (pos[t].max(axis=0) >= clo).all():
                            index = x + rx * (y + z * rz)
                            if index < g.cells.size:
                                want.add((index, t))
                            else:
                                dropped += 1
        assert listed == want and dropped > 0  # (res.z > res.y: the top of the box indexes past the array)
    for res in grid_rays.TIGHT_RES:  # tight lists: every triangle in the one cell that holds its centroid, or in none when that cell's index is past the array
        g = grid_rays.hand_grid(mesh, res, tight=True)
        rx, ry, rz = res
        seen = {}
        for c in range(g.cells.size):
            off = int(g.cells[c])
            for t in g.mapping_table[off + 1 : off + 1 + int(g.mapping_table[off])].tolist():
                assert t not in seen
                seen[t] = c
        pos = mesh.tri_pos.reshape(-1, 3, 3)
        for t in range(pos.shape[0]):
            x, y, z = (min(int(v), r - 1) for v, r in zip(np.floor((pos[t].sum(axis=0) / 3.0 - g.bbox_min) / g.cell_size), res))
            index = x + rx * (y + z * rz)
            assert seen.get(t) == (index if index < g.cells.size else None)
        assert len(seen) > pos.shape[0] // 3
