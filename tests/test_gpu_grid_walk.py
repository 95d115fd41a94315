"""Every form of the device's grid walk (raymond_amd/csrc/grid_walk.hpp) against the oracle's AccGrid::intersects, ray by ray, on adversarial rays.

One reference loop (acc_grid.rs:89-185) has become three stepping loops (the lean and the guarded assembly loop, the C++ loop of coarse masks), two
test distributions (the plain chunk() form and the DEEP form of the split / queued launches: sphere pre-test, the ring in the wave's carry area, walks
put aside by cut_lanes / cut_round and taken up again) and derived tables the reference does not have (seven entry slots per cell, the first-cell
quotient through an exact reciprocal).  Renders reach them only with camera and bounce rays and with allowances; form-against-form identity cannot see
an error the forms share.  Here each form answers the ray classes of tests/grid_rays.py — on which tests/test_grid_rays_host.py holds the oracle to
the second reading of the source, bit for bit — on the stand-in, the reference's four meshes, a small lumpy sphere and seven hand-built grids: five with
res.z > res.y (the guarded loop's end-of-array test ends walks in the middle of the box there; res.x = 1 and res.y = 1 among them, and one of 2160
cells, whose mask the small budget makes coarse: the C++ loop's end-of-array test) and two that list
every triangle in one cell only (the answer then depends on exactly which cells a walk visits — on bounding-box lists a walk that strays into a
neighbouring cell finds nothing its own cell does not list, which hides, for one, the side a -0.0 component steps to):

  * hit equal on every ray, the triangle equal on every hit — no share left out;
  * t within 4 ulp of the oracle's (the bound of arithmetic-only device functions, tests/test_gpu_parity.py);
  * across the device's own forms and mask settings hit, triangle and the bits of t identical;
  * 0.05 < the oracle's hit share < 0.95 per (grid, class), so that both outcomes stay represented (all-miss classes: nonfinite, in_face).

Forms: the plain probe; DEEP without cuts; DEEP with the production cut (K = 7: cut_lanes 7, cut_round 14) and a harsh one (31, 62), one wave per 64
and per 512 rays.  Masks: exact, and RMD_TUNE_MASK_BUDGET = 256 where that makes the mask coarser than one bit per cell (grids of more than 2048
cells).  Every class runs as class-pure batches of whole waves (a wave whose rays all start inside a builder-made grid takes the lean loop, a wave of
on_box rays the guarded one) and all classes together as one shuffled batch (lean or guarded round by round, carried walks beside fresh ones).
"""
import numpy as np
import pytest

import grid_rays
from raymond_amd import abi, probe, render, scenes
from raymond_amd.scene import Grid, Mesh
from test_gpu_parity import ulp_diff
from test_grid_rays_host import BUILT, HAND, K, grid_only_scene, small_grid, small_mesh

pytestmark = pytest.mark.gpu

FORMS = (("plain",), ("deep", 0, 0, 64), ("deep", 7, 14, 64), ("deep", 7, 14, 512), ("deep", 31, 62, 64), ("deep", 31, 62, 512))
MASK_BUDGET = 256  # bytes: 64 words, so a mask of one bit per cell no longer fits a grid of more than 2048 cells


def the_grid(oracle, name):
    if name == "standin":
        return scenes.gold_dragon_standin(n=24).objects[1].geometry.grid
    return small_grid(oracle, name)


def whole_waves(rays):
    """padded to a multiple of 64 with its own first rays"""
    pad = -rays.shape[0] % 64
    return np.concatenate([rays, rays[:pad]]) if pad else rays


def batches_for(grid, name):
    """-> [(label, rays)]: every class as a batch of whole waves, then all classes as one shuffled batch; the rays are those of the host test"""
    by_class = grid_rays.adversarial_rays(grid, np.random.default_rng(1000 + len(name)), K)
    batches = [(cls, whole_waves(by_class[cls])) for cls in grid_rays.CLASSES]
    every = np.concatenate([by_class[cls] for cls in grid_rays.CLASSES])
    every = every[np.random.default_rng(7).permutation(every.shape[0])]
    batches.append(("shuffled", whole_waves(every)))
    return batches


def run_form(ctx, ds, form, rays):
    if form[0] == "plain":
        return probe.grid_intersect(ctx, ds, 0, rays)
    return probe.grid_intersect_deep(ctx, ds, 0, rays, cut_lanes=form[1], cut_round=form[2], rays_per_wave=form[3])


def hold_to_oracle(label, got, want):
    (dh, dt, dtri), (oh, ot, otri) = got, want
    bad = np.flatnonzero(dh != oh)
    assert bad.size == 0, "%s: hit differs on %d rays, first %d: device %d, oracle %d" % (label, bad.size, bad[0], dh[bad[0]], oh[bad[0]])
    m = oh == 1
    bad = np.flatnonzero(m & (dtri != otri))
    assert bad.size == 0, "%s: triangle differs on %d hits, first %d: device %d (t %r), oracle %d (t %r)" % (
        label, bad.size, bad[0], dtri[bad[0]], dt[bad[0]], otri[bad[0]], ot[bad[0]])
    if m.any():
        u = ulp_diff(dt[m], ot[m])
        assert u.max() <= 4, "%s: t is %d ulp from the oracle's" % (label, u.max())


@pytest.mark.parametrize("name", ("standin",) + BUILT + HAND)
def test_every_form_of_the_walk_equals_the_oracle_on_adversarial_rays(gpu_ctx, oracle, name):
    grid = the_grid(oracle, name)
    scene = grid_only_scene(grid)
    osc = oracle.OracleScene(scene)
    batches = batches_for(grid, name)
    wants = []
    for label, rays in batches:
        want = osc.grid_intersect(0, rays)
        wants.append(want)
        if label in grid_rays.CLASSES and label not in grid_rays.ALL_MISS:
            assert 0.05 < want[0][:K].mean() < 0.95, (name, label, want[0][:K].mean())
    n_cells = int(grid.cells.size)
    first = {}  # batch label -> the first device answer: every other form and mask setting must give its bits
    legs = 0
    for budget in (0, MASK_BUDGET):
        gpu_ctx.set_tunable(abi.RMD_TUNE_MASK_BUDGET, budget)
        try:
            ds = render.DeviceScene(gpu_ctx, scene)
        finally:
            gpu_ctx.set_tunable(abi.RMD_TUNE_MASK_BUDGET, 0)
        try:
            _, n_grids, mask_words = probe.scene_layout(ds)
            assert n_grids == 1
            exact_words = (n_cells + 31) // 32 + 1  # one bit per cell and the zero word that ends every mask
            if budget == 0:
                assert mask_words >= exact_words, "the default budget holds these grids' exact masks"
            elif n_cells <= MASK_BUDGET * 8:
                continue  # the exact mask fits the small budget too: nothing new on this leg
            else:
                assert mask_words <= MASK_BUDGET // 4 < exact_words, "the mask is coarser than one bit per cell"
            legs += 1
            for form in FORMS:
                for (label, rays), want in zip(batches, wants):
                    got = run_form(gpu_ctx, ds, form, rays)
                    tag = "%s, mask budget %d, form %s, batch %s" % (name, budget, form, label)
                    hold_to_oracle(tag, got, want)
                    if label not in first:
                        first[label] = got
                    else:
                        h0, t0, tri0 = first[label]
                        assert np.array_equal(got[0], h0) and np.array_equal(got[2], tri0) and got[1].tobytes() == t0.tobytes(), tag + ": differs from the first form's bits"
        finally:
            ds.close()
    assert legs == (2 if n_cells > MASK_BUDGET * 8 else 1)


@pytest.mark.parametrize("name", ("standin",) + BUILT)
def test_scene_intersect_equals_the_oracle_on_adversarial_rays(gpu_ctx, oracle, name):
    """The same rays through Scene::intersect on the room around each builder-made grid: the walk behind scene_intersect_wave's box pre-check, merged
    with the planes and the sphere — object, triangle and t against the oracle."""
    if name == "standin":
        scene = scenes.gold_dragon_standin(n=24)
    else:
        mesh = small_mesh(name)  # (baked already)
        grid = small_grid(oracle, name)
        scene = scenes.mesh_scene(Mesh(mesh.tri_pos, mesh.tri_nrm), translate=(0.0, 0.0, 0.0), grid_builder=lambda m: grid)
    grid = scene.objects[1].geometry.grid
    assert isinstance(scene.objects[1].geometry, Grid)
    osc = oracle.OracleScene(scene)
    ds = render.DeviceScene(gpu_ctx, scene)
    try:
        on_grid = 0
        for label, rays in batches_for(grid, name):
            dobj, dt, dsub = probe.scene_intersect(gpu_ctx, ds, rays)
            oobj, ot, osub = osc.scene_intersect(rays)
            tag = "%s, batch %s" % (name, label)
            bad = np.flatnonzero(dobj != oobj)
            assert bad.size == 0, "%s: object differs on %d rays, first %d: device %d, oracle %d" % (tag, bad.size, bad[0], dobj[bad[0]], oobj[bad[0]])
            m = oobj == 1
            assert np.array_equal(dsub[m], osub[m]), tag + ": triangle differs"
            h = oobj >= 0
            if h.any():
                assert ulp_diff(dt[h], ot[h]).max() <= 4, tag
            on_grid += int(m.sum())
        assert on_grid > K  # the mesh is what many of these rays see first
    finally:
        ds.close()


def test_the_deep_probe_refuses_what_its_wave_loop_cannot_serve(gpu_ctx, oracle):
    """rays_per_wave that is no multiple of 64, cuts that do not fit the launch parameters' bytes, a grid the scene does not have: RMD_ERR_INVALID_ARGUMENT,
    no launch; and an empty batch is an empty answer."""
    from raymond_amd.lib import RaymondError

    grid = small_grid(oracle, "cube")
    ds = render.DeviceScene(gpu_ctx, grid_only_scene(grid))
    try:
        rays = batches_for(grid, "cube")[0][1]
        for kw in ({"rays_per_wave": 0}, {"rays_per_wave": 100}, {"rays_per_wave": 1 << 21}, {"cut_lanes": 256}, {"cut_round": 256}, {"g": 1}):
            args = {"g": 0, "cut_lanes": 0, "cut_round": 0, "rays_per_wave": 64}
            args.update(kw)
            with pytest.raises(RaymondError) as e:
                probe.grid_intersect_deep(gpu_ctx, ds, args.pop("g"), rays, **args)
            assert e.value.status == abi.RMD_ERR_INVALID_ARGUMENT, kw
        h, t, tri = probe.grid_intersect_deep(gpu_ctx, ds, 0, np.zeros((0, 6)))
        assert h.size == 0 and t.size == 0 and tri.size == 0
    finally:
        ds.close()
