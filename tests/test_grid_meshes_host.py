"""The adversarial meshes of tests/grid_meshes.py on the CPU.

  * the oracle's AccGrid::build_from_mesh equals the second reading of the source (tests/second_reading.py: grid_build) — status, bounds with their
    zero signs, resolution, cell size, cells, mapping table — on every mesh but the two largest (standin, big: a plain-Python build of 10^5
    triangles takes minutes).  This is what makes the oracle a reference for these meshes before tests/test_gpu_grid_build.py holds the device to it;
  * the host builder (rmd_grid_build_from_mesh) equals the oracle on every mesh in the sense of tests/test_grid_build.py::_equal, or both report
    status 5;
  * the generator's own claims are asserted from the oracle's tables, so that a later change to the generator cannot hollow the GPU leg out.

No tolerance appears anywhere: every comparison is equality of bytes."""
import functools

import numpy as np
import pytest

import grid_meshes
import second_reading as sr
from raymond_amd import abi, lib
from raymond_amd.scene import AccGrid
from test_grid_build import _equal

SEED = 20261016
NAMES = ("single", "few", "scan_1024", "scan_1023", "scan_1025") + tuple("scan_r%d" % i for i in range(len(grid_meshes.RESIDUE_SOUPS))) + (
    "zero_min_pos_neg", "zero_min_neg_pos", "zero_max_pos_neg", "zero_max_neg_pos", "beyond_max_seeds", "beyond_min_seed", "nan_vertex", "nan_triangle",
    "inf_vertex", "on_planes", "cluster", "spanning", "huge_1e100", "huge_1e103", "tiny_1e-105", "tiny_1e-300", "q5_panic", "standin", "big")


@functools.lru_cache(maxsize=None)
def the_meshes():
    """the set every test of the two legs uses (made once per process: `big` alone takes a second)"""
    return grid_meshes.adversarial_meshes(np.random.default_rng(SEED))


@functools.lru_cache(maxsize=None)
def oracle_grid(name):
    """-> (status, AccGrid or None) of the oracle's build"""
    import oracle_lib

    return oracle_lib.grid_build(the_meshes()[name])


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def test_the_generator_is_deterministic_and_complete():
    a, b = the_meshes(), grid_meshes.adversarial_meshes(np.random.default_rng(SEED))
    assert tuple(a) == NAMES == tuple(b)
    for name in NAMES:
        assert a[name].tri_pos.tobytes() == b[name].tri_pos.tobytes() and a[name].tri_nrm.tobytes() == b[name].tri_nrm.tobytes(), name
        assert np.isfinite(a[name].tri_nrm).all(), name
    assert set(grid_meshes.FAILING) < set(NAMES) and set(grid_meshes.SLOW_IN_PYTHON) < set(NAMES)


@pytest.mark.parametrize("name", [n for n in NAMES if n not in grid_meshes.SLOW_IN_PYTHON])
def test_oracle_equals_the_second_reading_of_the_builder(oracle, name):
    mesh = the_meshes()[name]
    rc, og = oracle_grid(name)
    try:
        s = sr.grid_build([tuple(map(float, p)) for p in mesh.tri_pos])
    except sr.Panic:
        assert rc == 5, "the second reading panics, the oracle builds"
        assert name in grid_meshes.FAILING
        return
    assert rc == 0, "the second reading builds, the oracle reports %d" % rc
    assert name not in grid_meshes.FAILING
    assert tuple(int(v) for v in og.resolution) == s["resolution"]
    assert bits(og.bbox_min) == bits(s["bbox_min"]) and bits(og.bbox_max) == bits(s["bbox_max"]), (og.bbox_min, og.bbox_max, s["bbox_min"], s["bbox_max"])
    assert bits(og.cell_size) == bits(s["cell_size"])
    assert og.cells.tolist() == s["cells"]
    assert og.mapping_table.tolist() == s["mapping_table"]


@pytest.mark.parametrize("name", NAMES)
def test_host_builder_equals_the_oracle(oracle, product_lib, name):
    mesh = the_meshes()[name]
    rc, og = oracle_grid(name)
    assert (rc == 5) == (name in grid_meshes.FAILING) and rc in (0, 5)
    if rc == 5:
        with pytest.raises(lib.RaymondError) as e:
            AccGrid.build_from_mesh(mesh)
        assert e.value.status == abi.RMD_ERR_GRID_INDEX
        return
    _equal(AccGrid.build_from_mesh(mesh), og)


def test_the_signed_zero_meshes_reach_both_signs(oracle):
    """the convention: the later zero of the fold wins — so each order ends on the other sign, for the minimum and for the maximum"""
    want = {"zero_min_pos_neg": ("bbox_min", -0.0), "zero_min_neg_pos": ("bbox_min", 0.0), "zero_max_pos_neg": ("bbox_max", -0.0),
            "zero_max_neg_pos": ("bbox_max", 0.0)}
    for name, (field, zero) in want.items():
        pos = the_meshes()[name].tri_pos
        v = pos.reshape(-1, 3)
        zeros = np.flatnonzero((v == 0.0).all(axis=1))
        assert zeros.size == 2 and (np.signbit(v[zeros[0]]) != np.signbit(v[zeros[1]])).all(), name
        other = np.delete(v, zeros, axis=0)
        assert (other > 0.0).all() if field == "bbox_min" else (other < 0.0).all(), name
        rc, og = oracle_grid(name)
        assert rc == 0 and bits(getattr(og, field)) == bits([zero] * 3), (name, getattr(og, field))


def test_the_generator_keeps_its_promises(oracle):
    """what tests/test_gpu_grid_build.py relies on, read from the oracle's tables"""
    meshes = the_meshes()
    built = {n: oracle_grid(n)[1] for n in NAMES if oracle_grid(n)[0] == 0}
    assert set(NAMES) - set(built) == set(grid_meshes.FAILING)
    n_cells = {n: int(g.cells.size) for n, g in built.items()}
    assert n_cells["single"] == 1 and built["single"].mapping_table.tolist() == [1, 0] and len(meshes["single"]) == 1
    assert tuple(built["few"].resolution) == (2, 2, 2) and len(meshes["few"]) == 3
    assert n_cells["scan_1024"] == 1024 and n_cells["scan_1023"] == 1023 and n_cells["scan_1025"] == 1025
    small = [n_cells["scan_r%d" % i] for i in range(len(grid_meshes.RESIDUE_SOUPS))]
    assert {c % 4 for c in small} == {0, 1, 2, 3} and {c % 4 for c in small if c < 256} == {0, 1, 2, 3}, small
    assert len(meshes["big"]) > 262144 and len(meshes["standin"]) == 99372
    assert n_cells["big"] > 512 * 1024  # hundreds of scan blocks
    # a bound that is a seed; a run that lists a triangle twice
    assert bits(built["beyond_max_seeds"].bbox_max) == bits(grid_meshes.SEED_MAX)
    assert built["beyond_min_seed"].bbox_min[0] == grid_meshes.SEED_MIN[0]
    assert bits(built["huge_1e100"].bbox_min) == bits(grid_meshes.SEED_MIN)
    twice = 0
    for name in ("beyond_max_seeds", "beyond_min_seed", "scan_1023"):
        g = built[name]
        for c in range(g.cells.size):
            off = int(g.cells[c])
            ids = g.mapping_table[off + 1 : off + 1 + int(g.mapping_table[off])]
            twice += int(np.unique(ids).size < ids.size)
    assert twice > 0
    assert grid_meshes.runs(built["beyond_max_seeds"]).max() > len(meshes["beyond_max_seeds"])  # longer than the mesh
    # the NaN coordinate is skipped: the bounds are the box
    assert np.isnan(meshes["nan_vertex"].tri_pos).sum() == 1 and np.isfinite(built["nan_vertex"].bbox_min).all() and np.isfinite(built["nan_vertex"].bbox_max).all()
    assert np.isnan(meshes["nan_triangle"].tri_pos).sum() == 3 and np.isinf(meshes["inf_vertex"].tri_pos).sum() == 1
    # on_planes: every vertex is a lattice value bbox_min + k * cell_size as binary64 computes it, and few of them lie on the box
    g = built["on_planes"]
    v = meshes["on_planes"].tri_pos.reshape(-1, 3)
    k = np.rint((v - g.bbox_min[None, :]) / g.cell_size[None, :])
    on = g.bbox_min[None, :] + k * g.cell_size[None, :] == v
    on[0], on[-1] = True, True  # the two bounding corners are the bounds themselves
    assert on.all() and (k >= 0).all() and (k <= g.resolution[None, :]).all()
    assert ((k > 0) & (k < g.resolution[None, :])).mean() > 0.7
    # cluster: one cell holds more than 512 triangles; spanning: one triangle is listed in every cell
    assert grid_meshes.runs(built["cluster"]).max() >= 512
    assert built["spanning"].mapping_table.size - built["cluster"].mapping_table.size > 7000
    # huge_1e100: every triangle reaches back to the origin cell, whose run is the whole mesh
    assert int(built["huge_1e100"].mapping_table[0]) == len(meshes["huge_1e100"])
    # THE SAFETY CONDITION of the GPU leg: the device sorts a run by insertion in one lane
    for name, g in built.items():
        assert grid_meshes.runs(g).max() <= grid_meshes.MAX_RUN, (name, grid_meshes.runs(g).max())
