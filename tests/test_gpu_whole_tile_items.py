"""Whole-tile work items of the role-sorted spheres kernel (raymond_amd/csrc/work_list.hpp, render_kernel.hpp: finish_sample_range), on the GPU.

In automatic mode a split persistent launch of a scene without grids runs the FIRST wave tiles of its list as one item each — all samples of the
pass on one wave, which adds them itself behind a wavefront-scope release / acquire — and splits only the last 2.5 tiles per wave slot.  A forced
RMD_TUNE_SAMPLE_SPLIT keeps the uniform split (K = 2, 4) or the direct mode (K = 1).  Every route adds the same samples in the same order, so the
frames are the same bytes.

The frame is C2's scene at 640 pixels across and just tall enough that the list has about 1,000 whole tiles beside its tail (the tail's size is
asked of the library: rmd_probe_work_plan with this context) — both kinds of item exist, which every case asserts.  Cases: 128 samples per pixel
(kSortedMinSamples: tail tiles of two parts) and 200 (three), with black paths ended and traced, with moments (sums and squares), a ragged frame
(width and height no multiples of 8: the host tiles arrive column by column, so the ragged bottom tiles of the first columns are whole items and
those of the last columns and the whole right edge are tail items), sample_begin != 0, accumulation into a non-zero framebuffer, two passes
(RMD_TUNE_SCRATCH_CAP_MB), and a tile list short enough to be all tail.  rmd_last_launch_info must report what the plan promises: buffered,
persistent, split_k = k_tail, the passes.

In the DIAG build RMD_DEBUG bit 1024 makes the tail 4 wave tiles, so that a 64x64 frame (64 wave tiles: 60 whole items) runs both kinds in a
persistent launch of its own; the same comparison there."""
import os
import subprocess
import sys

import numpy as np
import pytest

from raymond_amd import abi, probe, render, scenes
from raymond_amd.scene import Settings, generate_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "raymond_amd", "csrc", "diag", "libraymond_hip.so")
WIDTH = 640
FORCED = (2, 4, 1)  # the uniform split in two and in four items per wave tile, and the direct mode


@pytest.fixture(scope="module")
def ctx(product_lib):
    """A context of this module's own: the tests change its tunables."""
    with render.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def tail_tiles(ctx):
    """wave tiles of the list's tail on this device: what the plan leaves of a list far longer than it"""
    n_whole, n_tail, _ = probe.work_plan(0, 1 << 20, 200, 0, ctx=ctx)
    assert int(n_whole) > 0 and int(n_whole) + int(n_tail) == 1 << 20
    return int(n_tail)


def height_for(n_wave_tiles):
    return 8 * -(-n_wave_tiles // (WIDTH // 8))


def wave_tiles_of(W, H):
    return -(-W // 8) * -(-H // 8)  # (host tiles are 32x32, multiples of the wave tile: no wave tile is cut by a host tile's edge)


# name: (samples, Settings flags, moments, ragged, sample_begin, non-zero framebuffer, passes, all tail)
CASES = {
    "spp128": (128, {}, False, False, 0, False, 1, False),
    "spp200": (200, {}, False, False, 0, False, 1, False),
    "trace_black_paths_128": (128, {"trace_black_paths": True}, False, False, 0, False, 1, False),
    "trace_black_paths_200": (200, {"trace_black_paths": True}, False, False, 0, False, 1, False),
    "moments": (200, {}, True, False, 0, False, 1, False),
    "ragged": (200, {}, False, True, 0, False, 1, False),
    "sample_begin": (128, {}, False, False, 37, False, 1, False),
    "accumulate": (128, {}, False, False, 0, True, 1, False),
    "two_passes": (200, {}, False, False, 0, False, 2, False),
    "all_tail": (200, {}, False, False, 0, False, 1, True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_the_automatic_launch_equals_the_forced_splits_and_the_direct_mode_byte_for_byte(ctx, tail_tiles, case):
    spp, flags, moments, ragged, begin, nonzero, passes, all_tail = CASES[case]
    W = WIDTH - 3 if ragged else WIDTH
    H = height_for(tail_tiles - 1024 if all_tail else tail_tiles + 1024) - (3 if ragged else 0)
    n_tiles = wave_tiles_of(W, H)
    st = Settings(scenes.camera(W, H), sample_count=spp, tile_size=(32, 32), bounce_limit=5, seed=scenes.SEED, **flags)
    cam = st.camera_settings
    tiles = generate_tiles(W, H, st.tile_size)
    base = np.random.default_rng(5).uniform(0.0, 3.0, (H, W, 3)) if nonzero else None
    ds, fb, fb_sq = render.DeviceScene(ctx, scenes.reflective_spheres()), render.Framebuffer(ctx, W, H), render.Framebuffer(ctx, W, H) if moments else None

    def run(k):
        ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, k)
        fb.upload(base) if nonzero else fb.zero()
        if moments:
            fb_sq.zero()
        render.render_tiles(ctx, ds, cam, st, tiles, fb, begin, spp, framebuffer_sq=fb_sq)
        return fb.download(), (fb_sq.download() if moments else None), ctx.last_launch_info()

    try:
        per_pass = spp
        if passes == 2:  # a scratch cap that holds 120-odd of the 200 samples: two passes, both of at least 64
            per_sample = n_tiles * 64 * 32
            cap_mb = (per_sample * 120 >> 20) + 1
            per_pass = (cap_mb << 20) // per_sample
            assert 120 <= per_pass < 136
            ctx.set_tunable(abi.RMD_TUNE_SCRATCH_CAP_MB, cap_mb)
        # what the plan promises
        n_whole, n_tail, k_tail = (int(v) for v in probe.work_plan(0, n_tiles, spp, 0, ctx=ctx, pass_samples=per_pass))
        last_k = int(probe.work_plan(0, n_tiles, spp, 0, ctx=ctx, pass_samples=spp - per_pass)[2]) if passes == 2 else k_tail
        print("%s: %dx%d, %d wave tiles = %d whole + %d tail of %d parts" % (case, W, H, n_tiles, n_whole, n_tail, k_tail))
        assert n_whole + n_tail == n_tiles
        if all_tail:
            assert n_whole == 0 and k_tail == min(spp // 64, 64)  # the uniform rule's k on a list this short: as many parts as keep 64 samples
        else:
            assert n_whole >= 1000 and n_tail == tail_tiles and k_tail == min(per_pass // 64, 4)
        auto, auto_sq, info = run(0)
        assert info.has_grid == 0 and info.buffered == 1 and info.persistent == 1 and info.passes == passes and info.split_k == last_k, (
            info.buffered, info.persistent, info.passes, info.split_k)
        assert info.end_black_paths == (0 if flags.get("trace_black_paths") else 1)
        assert np.isfinite(auto).all() and auto.max() > 0.0
        for k in FORCED:
            ref, ref_sq, rinfo = run(k)
            assert rinfo.buffered == (0 if k == 1 else 1) and rinfo.split_k == k
            print("  forced %d: %d of %d values differ, max |difference| %.3g" % (k, (auto != ref).sum(), auto.size, np.nanmax(np.abs(auto - ref))))
            assert np.array_equal(auto, ref), (case, k)
            if moments:
                assert np.array_equal(auto_sq, ref_sq) and auto_sq.max() > 0.0, (case, k)
        if nonzero:
            assert (auto >= base).all() and (auto > base).any()  # added to what was there
    finally:
        ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0)
        ctx.set_tunable(abi.RMD_TUNE_SCRATCH_CAP_MB, 0)
        fb.close(), ds.close()
        if fb_sq is not None:
            fb_sq.close()


DIAG_CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np
from raymond_amd import abi, lib, render, scenes
from raymond_amd.scene import Settings, generate_tiles

assert lib.LIB_PATH.endswith("diag/libraymond_hip.so"), lib.LIB_PATH
os.environ["RMD_DEBUG"] = "1024"  # the work list's tail is 4 wave tiles
with render.Context(0) as ctx:
    ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 2)  # persistent, however few the items
    for W, H, spp, flags in ((64, 64, 128, {}), (64, 64, 200, {"trace_black_paths": True}), (61, 59, 200, {})):
        st = Settings(scenes.camera(W, H), sample_count=spp, tile_size=(32, 32), bounce_limit=5, seed=scenes.SEED, **flags)
        ds, fb = render.DeviceScene(ctx, scenes.reflective_spheres()), render.Framebuffer(ctx, W, H)
        frames = []
        for k in (0, 2, 1):
            ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, k)
            fb.zero()
            render.render_tiles(ctx, ds, st.camera_settings, st, generate_tiles(W, H, st.tile_size), fb)
            info = ctx.last_launch_info()
            assert (info.persistent == 1 or k == 1) and info.buffered == (0 if k == 1 else 1) and info.split_k == (min(spp // 64, 4) if k == 0 else k), (k, info.split_k)
            frames.append(fb.download())
        assert np.array_equal(frames[0], frames[1]) and np.array_equal(frames[0], frames[2]) and frames[0].max() > 0.0
        fb.close(), ds.close()
print("whole items ok")
"""


def test_whole_and_tail_items_in_a_small_frame_in_the_diag_build(product_lib):
    assert os.path.exists(DIAG_LIB), "build the DIAG library: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, RAYMOND_HIP_LIB=DIAG_LIB)
    env.pop("RMD_DEBUG", None)
    r = subprocess.run([sys.executable, "-c", DIAG_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "whole items ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
