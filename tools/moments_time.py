#!/usr/bin/env python3
"""What the per-pixel second moments cost, and what adaptive tile sampling buys (one GPU, one call):

    python tools/moments_time.py [--runs 5] [--out profiles/<round>/moments_time.json] [--quick]

1. C2 (ReflectiveSpheres 1920x1080, 500 spp) and C3 (GoldDragon stand-in, flags 0) rendered alternately without and with moments
   (rmd_render_tiles / rmd_render_tiles_moments), `runs` frames each; kernel times from the context's events, median and spread.
2. ReflectiveSpheres 1920x1080, 16 samples per pass, up to 256 spp: render_tiled adaptively (a few thresholds) against uniformly.  Reported:
   samples spent, wall time, and RMSE against a 2,000 spp uniform frame of another seed — for the adaptive frame and for a uniform frame of
   (about) the same number of samples.
--quick: 2 runs, C3 at 100 spp, the quality part at 640x360 (a smoke of the tool itself).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402


def time_config(ctx, name, runs, spp=None):
    st = scenes.config_settings(name, spp=spp)
    cam = st.camera_settings
    W, H = cam.backbuffer_width, cam.backbuffer_height
    ds = render.DeviceScene(ctx, getattr(scenes, scenes.CONFIGS[name][0])())
    tiles = generate_tiles(W, H, st.tile_size)
    fb, fb_sq = render.Framebuffer(ctx, W, H), render.Framebuffer(ctx, W, H)
    ms = {"off": [], "on": []}
    try:
        for warm in ("off", "on"):  # first launches allocate the scratch and queues
            fb.zero(), fb_sq.zero()
            render.render_tiles(ctx, ds, cam, st, tiles, fb, framebuffer_sq=fb_sq if warm == "on" else None)
        frames = {}
        for r in range(runs):
            for mode in (("off", "on") if r % 2 == 0 else ("on", "off")):  # alternated: drift falls on both alike
                fb.zero(), fb_sq.zero()
                render.render_tiles(ctx, ds, cam, st, tiles, fb, framebuffer_sq=fb_sq if mode == "on" else None)
                ms[mode].append(ctx.last_kernel_ms())
                if r == 0:
                    frames[mode] = fb.download()
        same = frames["off"].tobytes() == frames["on"].tobytes()
    finally:
        fb.close(), fb_sq.close(), ds.close()

    def stats(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_pct": 100.0 * (max(v) - min(v)) / min(v), "runs_ms": v}

    off, on = stats(ms["off"]), stats(ms["on"])
    return {"config": name, "spp": st.sample_count, "off": off, "on": on, "ratio_on_off_median": on["median_ms"] / off["median_ms"], "accum_identical": same}


def uniform_frame(ctx, ds, st, tiles, spp, seed):
    s = Settings(st.camera_settings, sample_count=spp, tile_size=st.tile_size, bounce_limit=st.bounce_limit, seed=seed)
    cam = s.camera_settings
    fb = render.Framebuffer(ctx, cam.backbuffer_width, cam.backbuffer_height)
    try:
        render.render_tiles(ctx, ds, cam, s, tiles, fb)
        return fb.download() / float(spp)
    finally:
        fb.close()


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def quality(ctx, W, H, spp, spi, thresholds, ref_spp):
    sc = scenes.reflective_spheres()
    st = Settings(scenes.camera(W, H), sample_count=spp, tile_size=(32, 32), bounce_limit=5, seed=scenes.SEED, samples_per_iteration=spi)
    tiles = generate_tiles(W, H, st.tile_size)
    ds = render.DeviceScene(ctx, sc)
    try:
        ref = uniform_frame(ctx, ds, st, tiles, ref_spp, scenes.SEED + 1)  # another seed: its noise is independent of the frames measured
        out = {"width": W, "height": H, "max_spp": spp, "samples_per_iteration": spi, "reference_spp": ref_spp, "runs": []}
        for thr in [0.0] + list(thresholds):
            s = Settings(scenes.camera(W, H), sample_count=spp, tile_size=(32, 32), bounce_limit=5, seed=scenes.SEED, samples_per_iteration=spi,
                         adaptive_threshold=thr)
            t0 = time.time()
            h = render.render_tiled(sc, s)
            wall = time.time() - t0
            fin = [m.tile for m in h._messages if m.kind == "TileFinished"]
            spent = int(sum(t.width * t.height * t.sample_count for t in fin))
            h.async_await()
            img = h.await_()
            row = {"threshold": thr, "samples": spent, "spp_mean": spent / float(W * H), "wall_s": wall, "rmse": rmse(img, ref),
                   "tiles_early": sum(1 for t in fin if t.sample_count < spp), "tiles": len(fin)}
            if thr > 0.0:  # a uniform frame of (about) the same number of samples
                eq = max(1, int(round(spent / float(W * H))))
                row["uniform_equal_samples"] = {"spp": eq, "samples": eq * W * H, "rmse": rmse(uniform_frame(ctx, ds, st, tiles, eq, scenes.SEED), ref)}
            out["runs"].append(row)
            print(json.dumps(row), flush=True)
        return out
    finally:
        ds.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    runs = 2 if a.quick else a.runs
    res = {"timing": [], "quality": None}
    with render.Context(0) as ctx:
        for name, spp in (("C2", None), ("C3", 100 if a.quick else None)):
            r = time_config(ctx, name, runs, spp)
            print(json.dumps(r), flush=True)
            res["timing"].append(r)
        W, H = (640, 360) if a.quick else (1920, 1080)
        res["quality"] = quality(ctx, W, H, 256, 16, (0.5, 0.25, 0.1, 0.05), 2000)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
