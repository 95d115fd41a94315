"""The lobe-uniform shading trips of the role-sorted spheres kernel (raymond_amd/csrc/render_kernel.hpp: render_wave_sorted), on the GPU.

The role-sorted form parks a hit WITHOUT its surface normal, on one of two stacks by the lobe its next bounce samples, and shades a stack at a
time with the lobe a compile-time argument (device_core.hpp: shade_lobe<>).  The lane-per-path form (render_wave: launches below
kSortedMinSamples = 128 samples per pixel) keeps a path in its lane, carries the normal and runs next_ray's merged stream.  Both must give every
sample the same bits:

  * the frame of ONE launch of 160 samples per pixel (the role-sorted form, asserted through rmd_last_launch_info) equals, byte for byte, the same
    samples rendered by two consecutive launches of 80 into one framebuffer (the lane-per-path form, asserted likewise; rmd_render_tiles adds in
    sample order, so the sums are the same bits) — on the C2 scene at 64x40, at 20x12 (ragged wave tiles), 8x8 and 1x1 (stacks that never fill: the
    drain rule with a handful of hits), in a room whose every object is metal (the diffuse stack stays empty), in a room of non-black diffuse
    objects (both stacks in use, about half each), in a room of metal and diffuse objects side by side, at bounce limits 1, 2 and 16, with
    RMD_RENDER_TRACE_BLACK_PATHS, under the thin lens (C5's camera on the C2 scene), and through rmd_render_tiles_moments (sums and squares);
  * the C2 64x40 frame also agrees with the oracle's render at the per-pixel bar of tests/test_gpu_fullsize.py (its rel_close and its
    account_for_off_pixels, called as test_whole_frame_of_the_production_kernel_against_the_oracle calls them);
  * in the DIAG build (RMD_DEBUG bit 8) on that frame every parked hit is shaded once, in a trip of its own lobe — hits shaded by lobe equal hits
    parked by lobe — and both lobes' trip counts are non-zero.

Not covered: a material of metalness 0.5 (prob_d = 0.25).  The library's materials are Diffuse (metalness 0, prob_d 0.5) and Metal (metalness 1,
prob_d 0): api_scene.cpp derives the metalness from the kind and no entry point sets another value, so such a room cannot be built through the C-ABI."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from raymond_amd import render, scenes
from raymond_amd.scene import Material, Object, Plane, Scene, Settings, Sphere, generate_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "raymond_amd", "csrc", "diag", "libraymond_hip.so")
SPP = 160  # >= kSortedMinSamples: one launch of it runs the role-sorted form; its halves run the lane-per-path form


def room(material_of):
    """The reference room (ceiling light, six walls) with two spheres; material_of(i) gives object i's material (the ceiling stays the light)."""
    sc = Scene()
    geoms = [Sphere((-1.0, -0.5, 3.5), 0.5), Sphere((0.74, -0.25, 3.5), 0.75), Plane((0.0, -1.0, 0.0), (0.0, 1.0, 0.0)), Plane((0.0, 2.0, 0.0), (0.0, -1.0, 0.0)),
             Plane((0.0, 0.0, -2.0), (0.0, 0.0, 1.0)), Plane((0.0, 0.0, 5.0), (0.0, 0.0, -1.0)), Plane((-2.0, 0.0, 0.0), (1.0, 0.0, 0.0)), Plane((2.0, 0.0, 0.0), (-1.0, 0.0, 0.0))]
    for i, g in enumerate(geoms):
        sc.objects.append(Object(g, Material.Emission((1.5, 1.5, 1.5), (1.0, 1.0, 1.0), 0.27, 0.0) if i == 3 else material_of(i)))
    return sc


COLORS = [(1.0, 0.2, 0.1), (0.05, 0.25, 1.0), (0.75, 0.75, 0.75), None, (1.0, 1.0, 1.0), (0.3, 0.8, 0.4), (0.9, 0.6, 0.2), (0.5, 0.5, 0.9)]
SCENES = {
    "c2": scenes.reflective_spheres,
    "all_metal": lambda: room(lambda i: Material.Metal(COLORS[i], 0.05 + 0.1 * i)),
    "all_diffuse": lambda: room(lambda i: Material.Diffuse(COLORS[i], 0.05 + 0.1 * i)),
    "metal_and_diffuse": lambda: room(lambda i: (Material.Metal if i % 2 else Material.Diffuse)(COLORS[i], 0.05 + 0.1 * i)),
}
# name: (scene, width, height, bounce limit, Settings flags, moments)
CASES = {
    "c2_64x40": ("c2", 64, 40, 5, {}, False),
    "c2_20x12_ragged": ("c2", 20, 12, 5, {}, False),
    "c2_8x8": ("c2", 8, 8, 5, {}, False),
    "c2_1x1": ("c2", 1, 1, 5, {}, False),
    "all_metal": ("all_metal", 64, 40, 5, {}, False),
    "all_diffuse": ("all_diffuse", 64, 40, 5, {}, False),
    "metal_and_diffuse": ("metal_and_diffuse", 64, 40, 5, {}, False),
    "bounces_1": ("c2", 64, 40, 1, {}, False),
    "bounces_2": ("c2", 64, 40, 2, {}, False),
    "bounces_16": ("c2", 64, 40, 16, {}, False),
    "trace_black_paths": ("c2", 64, 40, 5, {"trace_black_paths": True}, False),
    "thin_lens": ("c2", 64, 40, 5, {"use_dof": True}, False),
    "moments": ("c2", 64, 40, 5, {}, True),
}


def settings_of(case):
    scene, W, H, bounces, flags, moments = CASES[case]
    aperture = scenes.CONFIGS["C5"][5] if flags.get("use_dof") else 0.0  # C5's camera: the thin lens
    return Settings(scenes.camera(W, H, aperture), sample_count=SPP, tile_size=(32, 32), bounce_limit=bounces, seed=scenes.SEED, **flags)


def render_in_launches(ctx, sc, st, launches, moments, sorted_form):
    """(sums, squares or None): the samples 0 .. SPP - 1 rendered in `launches` consecutive launches into one framebuffer, each in the form asked for."""
    cam = st.camera_settings
    W, H = cam.backbuffer_width, cam.backbuffer_height
    tiles = generate_tiles(W, H, st.tile_size)
    ds, fb = render.DeviceScene(ctx, sc), render.Framebuffer(ctx, W, H)
    fb_sq = render.Framebuffer(ctx, W, H) if moments else None
    try:
        per = SPP // launches
        for k in range(launches):
            render.render_tiles(ctx, ds, cam, st, tiles, fb, k * per, per, framebuffer_sq=fb_sq)
            info = ctx.last_launch_info()
            assert info.has_grid == 0 and info.buffered == (1 if sorted_form else 0), (k, info.buffered, info.split_k)
        return fb.download(), (fb_sq.download() if moments else None)
    finally:
        fb.close(), ds.close()
        if fb_sq is not None:
            fb_sq.close()


@pytest.fixture(scope="module")
def c2_frame(gpu_ctx):
    """The C2 scene at 64x40, 160 spp, 5 bounces in ONE launch (the role-sorted form): rendered once, shared, never written to."""
    frame, _ = render_in_launches(gpu_ctx, SCENES["c2"](), settings_of("c2_64x40"), 1, False, True)
    frame.setflags(write=False)
    return frame


@pytest.mark.parametrize("case", list(CASES))
def test_one_role_sorted_launch_equals_the_lane_per_path_launches_byte_for_byte(gpu_ctx, c2_frame, case):
    sc, st, moments = SCENES[CASES[case][0]](), settings_of(case), CASES[case][5]
    if case == "c2_64x40":
        one, one_sq = c2_frame, None
    else:
        one, one_sq = render_in_launches(gpu_ctx, sc, st, 1, moments, True)
    ref, ref_sq = render_in_launches(gpu_ctx, sc, st, 2, moments, False)
    assert one.dtype == np.float64 and ref.dtype == np.float64
    print("%s: %d of %d values differ, max |difference| %.3g, frame mean %.6g" % (case, (one != ref).sum(), one.size, np.nanmax(np.abs(one - ref)), one.mean()))
    assert np.array_equal(one, ref)
    assert np.isfinite(one).all() and one.max() > 0.0  # not a comparison of empty frames
    if moments:
        assert np.array_equal(one_sq, ref_sq) and one_sq.max() > 0.0


def test_the_c2_frame_agrees_with_the_oracle_at_the_suites_bar(gpu_ctx, oracle, c2_frame):
    from test_gpu_fullsize import account_for_off_pixels, rel_close  # the suite's per-pixel bar, as the whole-frame test applies it

    sc, st = SCENES["c2"](), settings_of("c2_64x40")
    cam = st.camera_settings
    tiles = generate_tiles(cam.backbuffer_width, cam.backbuffer_height, st.tile_size)
    ref = oracle.OracleScene(sc, fast=True).render_tiles(cam, st, tiles, threads=16)
    dev = np.array(c2_frame)
    ok = rel_close(dev, ref, 1e-9).all(axis=2)
    account_for_off_pixels(gpu_ctx, oracle, sc, st, cam, SPP, dev, ref, ok, "lobe trips C2 64x40 %d spp" % SPP)
    assert abs(np.nanmean(dev) - np.nanmean(ref)) <= 1e-4 * np.nanmean(ref)


DIAG_CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
from raymond_amd import lib, render, scenes
from raymond_amd.scene import Settings, generate_tiles

assert lib.LIB_PATH.endswith("diag/libraymond_hip.so"), lib.LIB_PATH
os.environ["RMD_DEBUG"] = "8"  # the event counters
with render.Context(0) as ctx:
    st = Settings(scenes.camera(64, 40), sample_count=%(spp)d, tile_size=(32, 32), bounce_limit=5, seed=scenes.SEED)
    ds, fb = render.DeviceScene(ctx, scenes.reflective_spheres()), render.Framebuffer(ctx, 64, 40)
    render.render_tiles(ctx, ds, st.camera_settings, st, generate_tiles(64, 40, st.tile_size), fb)
    info = ctx.last_launch_info()
    assert info.buffered == 1 and info.has_grid == 0
    fb.close(), ds.close()
print("lobe counters ok")
"""


def test_every_parked_hit_is_shaded_once_in_a_trip_of_its_lobe_in_the_diag_build(product_lib):
    assert os.path.exists(DIAG_LIB), "build the DIAG library: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, RAYMOND_HIP_LIB=DIAG_LIB)
    env.pop("RMD_DEBUG", None)
    r = subprocess.run([sys.executable, "-c", DIAG_CHILD % {"root": ROOT, "spp": SPP}], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "lobe counters ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    tot = dict(d_trips=0, d_shaded=0, g_trips=0, g_shaded=0, d_parked=0, g_parked=0)
    for line in r.stderr.splitlines():
        m = re.search(r"lobe trips: diffuse trips=(\d+) diffuse hits shaded=(\d+) ggx trips=(\d+) ggx hits shaded=(\d+) \| hits parked: diffuse=(\d+) ggx=(\d+)", line)
        if m:
            for k, v in zip(("d_trips", "d_shaded", "g_trips", "g_shaded", "d_parked", "g_parked"), m.groups()):
                tot[k] += int(v)
    print(tot, "lanes per shading trip: diffuse %.1f, GGX %.1f" % (tot["d_shaded"] / max(tot["d_trips"], 1), tot["g_shaded"] / max(tot["g_trips"], 1)))
    assert tot["d_trips"] > 0 and tot["g_trips"] > 0, (tot, r.stderr[-2000:])
    assert tot["d_shaded"] == tot["d_parked"] and tot["g_shaded"] == tot["g_parked"], tot
    assert tot["d_shaded"] + tot["g_shaded"] > 64 * 40 * SPP // 4  # a good share of the frame's samples is shaded at least once
    assert tot["d_shaded"] <= 64 * tot["d_trips"] and tot["g_shaded"] <= 64 * tot["g_trips"]
