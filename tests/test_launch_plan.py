"""The launch form of every scene the library admits, on the host (no GPU): render_kernel.hpp's plan_launch through rmd_probe_launch_plan.

A frame has the same bits in every launch form, and the library picks the form at run time from the LDS a workgroup needs: the object table
(128 bytes an object), the grids' occupancy masks, and one area per wave.  The plan must never ask for more LDS than a CU has (a launch that
does fails with RMD_ERR_HIP instead of rendering), and it must charge each wave the area of the kernel it launches — the queued wave's exactly
when the queued kernel runs.  Checked here for every instantiation, every object count up to the admission limit and mask word totals over the
whole mask budget, against a plain restatement of the rule built from the library's own sizes (rmd_probe_launch_sizes)."""
import numpy as np
import pytest

from raymond_amd import probe

TILES, BUFFERED, LIST = probe.MODE_TILES, probe.MODE_TILES_BUFFERED, probe.MODE_LIST
INSTANTIATIONS = [(mode, grid) for mode in (TILES, BUFFERED, LIST) for grid in (False, True)]
ALL_FLAGS = range(16)  # PLAN_QUEUES | PLAN_PERSIST | PLAN_CHAIN | PLAN_MOMENTS


def round4(m):
    return (m + 3) // 4 * 4


def lds_fixed(S, n, m):
    """the part of a workgroup's LDS every form has: the object table and the masks (rounded up to 4 words)"""
    return S["object"] * n + 4 * round4(m)


def admitted(n, m, grid):
    """check_render_args (api.cpp): one wave's area beside the table and the masks fits the budget — the spheres kernel's area is its pool"""
    S = probe.launch_sizes(TILES, grid)
    return lds_fixed(S, n, m) + S["wave"] + (0 if grid else S["sort_pool"]) <= S["budget"]


def max_objects(m, grid):
    S = probe.launch_sizes(TILES, grid)
    room = S["budget"] - 4 * round4(m) - S["wave"] - (0 if grid else S["sort_pool"])
    return room // S["object"] if room >= 0 else -1


def documented_rule(mode, grid, n, m, flags, n_waves, n_cus):
    """The rule as render_kernel.hpp documents it, restated from the sizes: persistence (asked for, tile modes) takes the largest workgroup of
    4 .. kPersistWaves waves that fits, charged the queued wave's area when queues are attached to a split launch of a scene with grids; when not
    even 4 waves fit, or persistence was not asked for, one wave per work item in workgroups of up to kGridWavesPerWg waves (scenes with grids)
    or of one, charged the unqueued kernel's area."""
    S = probe.launch_sizes(mode, grid)
    n, m, flags = (np.asarray(a, dtype=np.int64) for a in (n, m, flags))
    fixed = lds_fixed(S, n, m)
    budget = S["budget"]
    moments = ((flags & probe.PLAN_MOMENTS) != 0) & (mode == TILES or (mode == BUFFERED and not grid))
    persist = ((flags & probe.PLAN_PERSIST) != 0) & (mode != LIST)
    queued = ((flags & probe.PLAN_QUEUES) != 0) & (mode == BUFFERED and grid)
    pwave = np.where(queued, S["queued_wave"], S["wave"])
    pw = np.clip((budget - fixed) // pwave, 4, S["persist_waves"])
    persistent = persist & (fixed + pw * pwave <= budget)
    w = np.clip((budget - fixed) // S["wave"], 1, S["grid_waves"] if grid else 1)
    waves = np.where(persistent, pw, w)
    wave_lds = np.where(persistent, pwave, S["wave"])
    groups = -(-np.asarray(n_waves, dtype=np.int64) // waves)
    return {
        "persistent": persistent.astype(np.int64),
        "queued": (persistent & queued).astype(np.int64),
        "chained": (persistent & ~queued & ((flags & probe.PLAN_CHAIN) != 0) & (mode == BUFFERED and grid)).astype(np.int64),
        "moments": moments.astype(np.int64),
        "waves_per_wg": waves,
        "workgroups": np.where(persistent, np.minimum(groups, n_cus), groups),
        "wave_lds": wave_lds,
        "lds": fixed + waves * wave_lds,
    }


def windows(x):
    """sorted values -> the intervals they make up at the 16-byte grain of the layout: a failure names its windows of X"""
    x = np.unique(x)
    if x.size == 0:
        return []
    cut = np.nonzero(np.diff(x) > 16)[0]
    starts, ends = np.r_[x[0], x[cut + 1]], np.r_[x[cut], x[-1]]
    return [(int(a), int(b)) for a, b in zip(starts, ends)]


def scene_grid(grid):
    """(n_objects, mask_words_total) of every scene admitted to the instantiation, in fine steps: scenes without grids have no mask words; with
    grids every multiple of 4 words from 4 to the 48 KiB mask budget (rmd_scene_create rounds each grid's mask up to 4 words), the words in between
    at a coarser step, and the totals above the budget that many small grids reach, up to the admission edge"""
    if not grid:
        ms = np.array([0])
    else:
        S = probe.launch_sizes(TILES, True)
        budget_words = S["mask_budget"] // 4
        top = (S["budget"] - S["wave"]) // 4  # no object at all: the most mask words a scene may have
        ms = np.unique(np.r_[1, 2, 3, np.arange(4, budget_words + 1, 4), np.arange(5, budget_words, 97), np.arange(6, budget_words, 89), np.arange(7, budget_words, 83),
                             np.arange(budget_words, top + 1, 52), top - 3, top - 2, top - 1, top])
    ns, mm = [], []
    for m in ms:
        k = max_objects(int(m), grid)
        if k >= 0:
            ns.append(np.arange(0, k + 1)), mm.append(np.full(k + 1, m))
    return np.concatenate(ns), np.concatenate(mm)


@pytest.fixture(scope="module")
def sizes(product_lib):
    return {inst: probe.launch_sizes(*inst) for inst in INSTANTIATIONS}


def test_the_sizes_are_the_layouts_the_kernels_use(sizes):
    """The numbers the plan is made of, as the library has them: 128 bytes an object, a 160 KiB budget and a 48 KiB mask budget for every
    instantiation; the spheres kernel's wave is its pool and a 16-byte head, the lane-per-path kernel's without grids the head alone, and the
    queued wave of the mesh kernel holds more than its lane-per-path wave."""
    for (mode, grid), S in sizes.items():
        assert S["budget"] == 160 * 1024 and S["object"] == 128 and S["mask_budget"] == 48 * 1024, (mode, grid, S)
        assert S["grid_waves"] == 4 and 4 <= S["persist_waves"] <= 16
        assert S["wave"] % 16 == 0 and S["queued_wave"] % 16 == 0, S  # every per-wave area keeps the next one 16-byte aligned
        if grid:
            assert S["wave"] == sizes[(TILES, True)]["wave"] and S["queued_wave"] > S["wave"], S
        elif mode == BUFFERED:
            assert S["wave"] == sizes[(TILES, False)]["wave"] + S["sort_pool"], S  # render_wave_sorted: the pool, then the head
        else:
            assert S["wave"] == 16, S  # the lane-per-path kernel without grids: the head alone


@pytest.mark.parametrize("mode,grid", INSTANTIATIONS, ids=["%s-%s" % (("tiles", "buffered", "list")[m], "grid" if g else "spheres") for m, g in INSTANTIATIONS])
def test_every_admitted_scene_gets_a_launch_that_fits(sizes, mode, grid):
    S = sizes[(mode, grid)]
    n, m = scene_grid(grid)
    assert admitted(int(n[-1]), int(m[-1]), grid) and not admitted(int(n[-1]) + 1, int(m[-1]), grid)
    x = lds_fixed(S, n, m)
    order = np.argsort(x, kind="stable")
    n, m, x = n[order], m[order], x[order]
    n_waves, n_cus = 4096 * 64, 256
    # the flags an instantiation reads, over every scene; the ones it ignores over every 13th (they must change nothing either)
    read = (probe.PLAN_PERSIST if mode != LIST else 0) | (probe.PLAN_QUEUES | probe.PLAN_CHAIN if (mode == BUFFERED and grid) else 0)
    read |= probe.PLAN_MOMENTS if (mode == TILES or (mode == BUFFERED and not grid)) else 0
    full = (n, m, x)
    for flags in ALL_FLAGS:
        n, m, x = full if flags & ~read == 0 else (a[::13] for a in full)
        got = probe.launch_plan(mode, grid, n, m, flags, n_waves, n_cus)
        want = documented_rule(mode, grid, n, m, flags, n_waves, n_cus)
        where = "mode %d grid %d flags %d" % (mode, grid, flags)
        over = got["lds"] > S["budget"]
        assert not over.any(), "%s: the plan asks for more LDS than the budget at X in %s" % (where, windows(x[over]))
        # the per-wave area charged is the layout of the kernel launched: the queued wave's exactly when the queued kernel runs
        layout = np.where(got["queued"] == 1, S["queued_wave"], S["wave"])
        bad = got["wave_lds"] != layout
        assert not bad.any(), "%s: a wave charged at one layout and launched with the other at X in %s" % (where, windows(x[bad]))
        assert (got["lds"] == x + got["waves_per_wg"] * got["wave_lds"]).all(), where
        # waves per workgroup in range, and never more for a larger table
        p = got["persistent"] == 1
        w = got["waves_per_wg"]
        assert ((w[p] >= 4) & (w[p] <= S["persist_waves"])).all() and ((w[~p] >= 1) & (w[~p] <= (S["grid_waves"] if grid else 1))).all(), where
        up = np.nonzero(np.diff(w) > 0)[0]
        assert up.size == 0, "%s: more waves per workgroup for a larger table at X = %s" % (where, x[up[:8] + 1].tolist())
        assert (np.diff(got["persistent"]) <= 0).all(), where  # once a table is too large for the persistent form, so is every larger one
        # the kernels the flags allow, and only those
        assert not got["queued"][~p].any() and not got["chained"][~p].any() and not (got["queued"] & got["chained"]).any(), where
        if not (mode == BUFFERED and grid):
            assert not got["queued"].any() and not got["chained"].any(), where
        if mode == LIST or not flags & probe.PLAN_PERSIST:
            assert not p.any(), where
        for key in probe.PLAN_FIELDS:
            diff = got[key] != want[key]
            assert not diff.any(), "%s: %s differs from the documented rule at X in %s" % (where, key, windows(x[diff]))


@pytest.mark.parametrize("mode,grid", [(TILES, False), (TILES, True), (BUFFERED, False), (BUFFERED, True)])
def test_workgroups_of_each_form(sizes, mode, grid):
    """The launch grid: ceil(work items / waves per workgroup) workgroups, and no more persistent ones than the device has CUs."""
    n, m = scene_grid(grid)
    pick = np.unique(np.r_[0, np.linspace(0, n.size - 1, 257).astype(np.int64)])
    n, m = n[pick], m[pick]
    for n_waves in (1, 3, 63, 64, 65, 1000, 4096 * 64, 2**31 - 1):
        for n_cus in (1, 80, 256):
            for flags in (probe.PLAN_PERSIST, probe.PLAN_PERSIST | probe.PLAN_QUEUES | probe.PLAN_CHAIN, 0, probe.PLAN_MOMENTS | probe.PLAN_PERSIST):
                got = probe.launch_plan(mode, grid, n, m, flags, n_waves, n_cus)
                want = documented_rule(mode, grid, n, m, flags, n_waves, n_cus)
                assert (got["workgroups"] == want["workgroups"]).all(), (mode, grid, n_waves, n_cus, flags)
                assert (got["workgroups"] * got["waves_per_wg"] >= np.where(got["persistent"] == 1, np.minimum(n_waves, got["waves_per_wg"]), n_waves)).all()


def test_the_boundaries_of_the_mesh_kernel_sit_where_the_sizes_put_them(sizes):
    """The edges a GPU sweep (tests/test_gpu_launch_edges.py) renders either side of, from the sizes alone: a persistent split launch with path
    queues keeps 4 waves up to X = budget - 4 x the queued wave, and beyond it runs one wave per item — in workgroups of 4 while 4 unqueued waves
    fit, which is where the queued pricing of the fallback asked for more than the budget."""
    S = sizes[(BUFFERED, True)]
    B, Q, W = S["budget"], S["queued_wave"], S["wave"]
    x = np.arange(0, B - W + 1, 16)
    m = np.full(x.size, 4)
    n_obj = (x - 16) // 128
    keep = n_obj >= 0
    x, m, n_obj = x[keep], m[keep], n_obj[keep]
    exact = lds_fixed(S, n_obj, m) == x
    x, m, n_obj = x[exact], m[exact], n_obj[exact]
    got = probe.launch_plan(BUFFERED, True, n_obj, m, probe.PLAN_PERSIST | probe.PLAN_QUEUES | probe.PLAN_CHAIN, 4096 * 64, 256)
    assert (got["persistent"][x <= B - 4 * Q] == 1).all() and (got["persistent"][x > B - 4 * Q] == 0).all()
    for w in (4, 3, 2, 1):
        inside = (x > B - (w + 1) * W) & (x <= B - w * W) if w < 4 else (x > B - 4 * Q) & (x <= B - 4 * W)
        assert inside.any() and (got["waves_per_wg"][inside] == w).all() and (got["lds"][inside] <= B).all(), w
