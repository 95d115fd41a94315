"""Adversarial rays for the grid walk, and hand-built grids with res.z > res.y — plain numpy, no GPU, no oracle.

adversarial_rays(grid, rng, k) -> {class name: (k, 6) float64}: the ray classes on which a port of AccGrid::intersects (acc_grid.rs:89-185) goes wrong
without a render noticing — NaN and tied t_max, origins on lattice planes and on the box, zero / denormal / non-finite components, rays inside a box
face, rays through mesh vertices.  tests/test_grid_rays_host.py holds the oracle to the second reading of the source on every class (which is what makes
the oracle's answer a reference for them); tests/test_gpu_grid_walk.py then holds every form of the device's walk to the oracle.

Every direction is normalised AFTER its special components have been put in (the DEEP walk's sphere pre-test assumes |rd| = 1 to rounding), except in
the non-finite class.  `grid` is anything with bbox_min, bbox_max, cell_size, resolution and tri_pos (raymond_amd.scene.AccGrid).  A "lattice value" of
axis a is lo[a] + i * cs[a] as binary64 computes it, for an integer 0 <= i <= res[a].
"""
import numpy as np

from raymond_amd.scene import AccGrid

CLASSES = ("nan_tmax", "corner", "diag", "on_box", "tiny", "nonfinite", "in_face", "vertex", "plain", "neg_zero")
ALL_MISS = ("nonfinite", "in_face")  # classes whose rays the reference's walk never answers with a hit (measured; the tests assert device == oracle on them, no band)
TINY = (1e-300, -1e-300, 5e-324, -5e-324, 1e-17, -1e-17)
HAND_RES = ((4, 3, 6), (5, 2, 7), (1, 4, 9), (6, 1, 5), (12, 9, 20))  # (the last: more than 2048 cells, so that a small mask budget makes its mask coarse)
TIGHT_RES = ((4, 4, 4), (4, 3, 6))  # hand-built grids whose cells list a triangle in one cell only (hand_grid(..., tight=True))


def _normalise(d):
    with np.errstate(all="ignore"):
        return d / np.sqrt((d * d).sum(axis=1))[:, None]


def _box(grid):
    lo, hi = np.asarray(grid.bbox_min, dtype=np.float64), np.asarray(grid.bbox_max, dtype=np.float64)
    cs = np.asarray(grid.cell_size, dtype=np.float64)
    res = np.asarray(grid.resolution).astype(np.int64)
    return lo, hi, cs, res


def _walkable(lo, hi, cs, res):
    """The part of the box whose cells have an index inside the cell array: with the reference's index x + res.x * (y + z * res.z) (Q5) that is the
    layers z < res.y — the whole box for every grid the builder makes (res.z <= res.y), a slab at the bottom for a hand-built one, where a walk that
    enters or reaches a higher layer ends (acc_grid.rs:129-131).  -> (hi of that part, its resolution)"""
    wres = res.copy()
    wres[2] = min(res[2], res[1])
    whi = hi.copy()
    if wres[2] < res[2]:
        whi[2] = lo[2] + float(wres[2]) * cs[2]
    return whi, wres


def _lattice(lo, cs, res, rng, k, boundary=None):
    """(k, 3) lattice corners lo + i * cs (i uniform in 0..res; boundary=True: i in {0, res} only), and i"""
    if boundary:
        i = rng.integers(0, 2, (k, 3)) * res[None, :]
    else:
        i = rng.integers(0, res[None, :] + 1, (k, 3))
    return lo[None, :] + i.astype(np.float64) * cs[None, :], i


def _outside(lo, hi, rng, k, below=False):
    """origins on a shell around the box (lo, hi), 1.2 .. 3 half-diagonals from its centre; below=True: none of them above it (a ray from above a
    hand-built grid's walkable slab enters the box through a layer that is past the cell array, and ends there)"""
    centre, half = (lo + hi) / 2, np.sqrt(((hi - lo) ** 2).sum()) / 2
    u = _normalise(rng.normal(size=(k, 3)))
    if below:
        u[:, 2] = -np.abs(u[:, 2])
    return centre[None, :] + u * (half * rng.uniform(1.2, 3.0, (k, 1)))


def _aim(o, target):
    return np.concatenate([o, _normalise(target - o)], axis=1)


def adversarial_rays(grid, rng, k):
    lo, box_hi, cs, box_res = _box(grid)
    # targets, inner origins and lattice corners are drawn from the part of the box a walk can cross (the whole box unless res.z > res.y), so that the
    # classes keep both outcomes on the hand-built grids too; the faces of on_box / in_face are those of the box itself
    hi, res = _walkable(lo, box_hi, cs, box_res)
    slab = bool(res[2] < box_res[2])
    centre, size = (lo + hi) / 2, hi - lo
    out = {}
    rows = np.arange(k)

    # nan_tmax: origin inside the box with one coordinate a lattice value, the direction's component on that axis +0.0 or -0.0: t_max = 0 / 0 there
    # (every compare of the axis choice is false) or +-inf, and signum(-0.0) = -1
    o = centre + rng.uniform(-0.45, 0.45, (k, 3)) * size
    axis = rng.integers(0, 3, k)
    lat, _ = _lattice(lo, cs, res, rng, k)
    o[rows, axis] = lat[rows, axis]
    d = (centre + rng.uniform(-0.5, 0.5, (k, 3)) * size) - o
    d[rows, axis] = 0.0
    d = _normalise(d)
    d[rows, axis] = np.where(rng.integers(0, 2, k) == 0, 0.0, -0.0)
    out["nan_tmax"] = np.concatenate([o, d], axis=1)

    # corner: from outside, aimed exactly at a lattice corner: ties and near-ties of two and three t_max
    # (every other one from the far side, through a point inside: where all corners lie on the box — a resolution of 1 — the first kind only grazes it)
    lat, _ = _lattice(lo, cs, res, rng, k)
    o = _outside(lo, hi, rng, k, below=slab)
    inner_pt = centre + rng.uniform(-0.45, 0.45, (k, 3)) * size
    half_diag = np.sqrt((size * size).sum()) / 2
    through = inner_pt + _normalise(inner_pt - lat) * (half_diag * rng.uniform(2.0, 3.0, (k, 1)))
    o[1::2] = through[1::2]
    out["corner"] = _aim(o, lat)

    # diag: origin ON a lattice corner (every fourth one a corner of the box), direction normalize(+-cs): exact ties step after step, and a first-cell
    # quotient that is an exact integer
    # (a corner on the top of a hand-built grid's walkable slab belongs to the layer above it, where no walk starts: one layer less there)
    inner = res - np.array([0, 0, 1]) if slab else res
    lat, _ = _lattice(lo, cs, inner, rng, k)
    latb, _ = _lattice(lo, cs, inner, rng, k, boundary=True)
    lat[::4] = latb[::4]
    sign = np.where(rng.integers(0, 2, (k, 3)) == 0, 1.0, -1.0)
    out["diag"] = np.concatenate([lat, _normalise(sign * cs[None, :])], axis=1)

    # on_box: origin on a face, an edge or a corner of the box (1, 2 or 3 coordinates equal to lo or hi), aimed inside: t_outer = 0, the start cell
    # res[a] on the max side (Q6), the re-base of a negative first cell
    o = centre + rng.uniform(-0.5, 0.5, (k, 3)) * size
    n_fixed = 1 + rows % 3
    order = np.argsort(rng.uniform(size=(k, 3)), axis=1)
    side = rng.integers(0, 2, (k, 3))
    for j in range(3):
        a = order[:, j]
        fix = j < n_fixed
        o[rows[fix], a[fix]] = np.where(side[fix, j] == 0, lo[a[fix]], box_hi[a[fix]])
    out["on_box"] = _aim(o, centre + rng.uniform(-0.55, 0.55, (k, 3)) * size)

    # tiny: aimed at the box, then one component replaced by a tiny or denormal value and renormalised: t_delta and t_max huge or infinite
    o = _outside(lo, hi, rng, k, below=slab)
    d = _normalise((centre + rng.uniform(-0.3, 0.3, (k, 3)) * size) - o)
    axis = rng.integers(0, 3, k)
    d[rows, axis] = np.asarray(TINY)[rng.integers(0, len(TINY), k)]
    d = _normalise(d)
    # keep the origin in front of the box along the remaining components: move the replaced coordinate of the origin into the box's range, where
    # the ray (now parallel to that axis' planes, for all that binary64 can tell) can meet the mesh
    o[rows, axis] = centre[axis] + rng.uniform(-0.3, 0.3, k) * size[axis]
    out["tiny"] = np.concatenate([o, d], axis=1)

    # nonfinite: a corner ray with one of its six numbers NaN, +inf or -inf (NOT normalised again)
    lat, _ = _lattice(lo, cs, res, rng, k)
    r = _aim(_outside(lo, hi, rng, k, below=slab), lat)
    r[rows, rng.integers(0, 6, k)] = np.asarray([np.nan, np.inf, -np.inf])[rng.integers(0, 3, k)]
    out["nonfinite"] = r

    # in_face: origin in the plane of a box face — inside and outside the face's rectangle — direction inside that plane: the slab test's 0 * inf,
    # walks along the outermost cell layer
    axis = rng.integers(0, 3, k)
    o = centre + rng.uniform(-0.5, 0.5, (k, 3)) * size
    far = rows % 2 == 1
    o[far] = centre + rng.uniform(-1.5, 1.5, (int(far.sum()), 3)) * size
    o[rows, axis] = np.where(rng.integers(0, 2, k) == 0, lo[axis], box_hi[axis])
    tgt = centre + rng.uniform(-0.5, 0.5, (k, 3)) * size
    d = tgt - o
    d[rows, axis] = 0.0
    d = _normalise(d)
    d[rows, axis] = np.where(rng.integers(0, 2, k) == 0, 0.0, -0.0)
    out["in_face"] = np.concatenate([o, d], axis=1)

    # vertex: aimed exactly at a mesh vertex from 1, 1e3 and 1e6 away: hits on edges and vertices (first-wins ties between the triangles of a fan), the
    # pre-test's distance-proportional allowance in situ
    verts = np.asarray(grid.tri_pos, dtype=np.float64).reshape(-1, 3)
    verts = verts[verts[:, 2] <= hi[2]]  # (all of them unless the walkable part is a slab)
    v = verts[rng.integers(0, verts.shape[0], k)]
    dist = np.asarray([1.0, 1e3, 1e6])[rows % 3]
    # from outside the mesh: away from the box's centre, give or take
    u = _normalise(_normalise(v - centre[None, :]) + rng.normal(scale=0.35, size=(k, 3)))
    o = v + u * dist[:, None]
    out["vertex"] = _aim(o, v)

    # plain: the classes the second reading's test already holds, for continuity
    from test_second_reading import rays_for

    r = rays_for(grid, rng, k)
    r[:, 3:] = _normalise(r[:, 3:])  # (rays_for zeroes a component of some unit vectors and leaves them short; zeros stay zeros)
    out["plain"] = r
    # neg_zero: one direction component -0.0: t_delta = -inf and t_max = -inf on that axis, so the walk steps along THAT axis until it leaves the
    # grid, towards the side signum(-0.0) = -1 names, testing the cells it crosses — cells the ray itself never enters.  Where cells list triangles by
    # their bounding boxes the first cell lists whatever those cells could add; on a grid with tight lists (hand_grid(..., tight=True)) the answer
    # depends on the side.  The ray lies in (or 1e-9 cells beside) a lattice plane next to the cell that holds a triangle's centroid, starts a
    # fraction of a cell away in that cell's row and heads for the centroid's projection onto the plane: it meets the triangle where that reaches across.
    tris = np.asarray(grid.tri_pos, dtype=np.float64).reshape(-1, 3, 3)
    cen = tris.sum(axis=1) / 3.0
    cen = cen[cen[:, 2] <= hi[2]]  # (all of them unless the walkable part is a slab)
    cen = cen[rng.integers(0, cen.shape[0], k)]
    axis = rows % 3
    cell = np.minimum(np.floor((cen - lo) / cs).astype(np.int64), box_res - 1)
    plane_i = cell[rows, axis] + (rows // 3) % 2
    tgt = cen.copy()
    tgt[rows, axis] = lo[axis] + plane_i.astype(np.float64) * cs[axis] + np.asarray([0.0, 1e-9, -1e-9])[(rows // 6) % 3] * cs[axis]
    u = rng.normal(size=(k, 3))
    u[rows, axis] = 0.0
    u = _normalise(u)
    o = tgt - u * (rng.uniform(0.05, 0.6, (k, 1)) * cs.min())
    d = u.copy()
    d[rows, axis] = -0.0
    out["neg_zero"] = np.concatenate([o, d], axis=1)
    assert tuple(out) == CLASSES and all(r.shape == (k, 6) for r in out.values())
    return out


def hand_grid(mesh, res, tight=False):
    """A grid description the builder never produces — a resolution with res.z > res.y (AccGrid::build_from_mesh panics on every such mesh), or
    tight lists — which rmd_scene_create and the oracle accept.  A test fixture with a stated rule, not a port of the builder: box = the vertices'
    bounds, cs = (hi - lo) / res, every triangle listed (ascending) in every cell its bounding box overlaps (closed intervals), at the reference's
    index x + res.x * (y + z * res.z) (Q5), references whose index is >= n_cells dropped.  tight=True: a triangle is listed in ONE cell, the one that holds its centroid
    (cell = floor((p - lo) / cs), at most res - 1) — a walk then finds a triangle only in that cell, wherever the ray meets it, so that the answer
    depends on exactly which cells the walk visits, and in which order."""
    res = np.asarray(res, dtype=np.int64)
    pos = np.asarray(mesh.tri_pos, dtype=np.float64).reshape(-1, 3, 3)
    lo, hi = pos.reshape(-1, 3).min(axis=0), pos.reshape(-1, 3).max(axis=0)
    cs = (hi - lo) / res
    n_cells = int(res[0] * res[1] * res[2])
    tmin, tmax = pos.min(axis=1), pos.max(axis=1)
    lists = [[] for _ in range(n_cells)]
    planes = [lo[a] + np.arange(res[a] + 1, dtype=np.float64) * cs[a] for a in range(3)]
    if tight:
        for ti in range(pos.shape[0]):
            c = np.minimum(np.floor((pos[ti].sum(axis=0) / 3.0 - lo) / cs).astype(np.int64), res - 1)
            index = int(c[0] + res[0] * (c[1] + c[2] * res[2]))
            if index < n_cells:
                lists[index].append(ti)
    for ti in range(pos.shape[0] if not tight else 0):
        rng_a = []
        for a in range(3):
            i = np.arange(res[a])
            rng_a.append(i[(planes[a][:-1] <= tmax[ti, a]) & (planes[a][1:] >= tmin[ti, a])])
        for z in rng_a[2]:
            for y in rng_a[1]:
                for x in rng_a[0]:
                    index = int(x + res[0] * (y + z * res[2]))
                    if index < n_cells:
                        lists[index].append(ti)
    cells, table = np.zeros(n_cells, dtype=np.uint32), []
    for c in range(n_cells):
        cells[c] = len(table)
        table.append(len(lists[c]))
        table.extend(lists[c])
    return AccGrid(lo, hi, res, cs, cells, np.asarray(table, dtype=np.uint32), mesh.tri_pos, mesh.tri_nrm)


def grid_dict(grid):
    """the grid as tests/second_reading.py takes it"""
    return {"bbox_min": tuple(map(float, grid.bbox_min)), "bbox_max": tuple(map(float, grid.bbox_max)), "cell_size": tuple(map(float, grid.cell_size)),
            "resolution": tuple(int(v) for v in grid.resolution), "cells": grid.cells.tolist(), "mapping_table": grid.mapping_table.tolist(),
            "tri_pos": [tuple(map(float, p)) for p in grid.tri_pos]}


def hit_share_in_band(hit):
    """both outcomes stay represented: 0.05 < the oracle's hit share < 0.95"""
    return 0.05 < float(np.mean(hit)) < 0.95
