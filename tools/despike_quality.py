#!/usr/bin/env python3
"""What rmd_despike does to a frame's error, and to adaptive sampling, on one GPU:

    python tools/despike_quality.py quality  [--out profiles/r23_despike/quality.json]
    python tools/despike_quality.py adaptive [--out profiles/r23_despike/adaptive.json]
    python tools/despike_quality.py tile_errors [--out profiles/r23_despike/tile_error_effect.json]

quality    256 x 144, 16 and 64 spp, both bundled scenes, 5 bounces, rmd_despike at the starting values (radius 2, rank 2, k 6, ratio 2, floor 0).  RMSE
           against a 2,048 spp frame of another seed for S / n, rmd_denoise (radius 10, patch 3, k 0.45) and rmd_denoise_atrous (5 levels, k 3), each on the
           raw sums and on the despiked ones; the share of pixels replaced; and the mean luminance the stage removed — its bias.
adaptive   DESIGN.md section 10's table again: ReflectiveSpheres 1920 x 1080, up to 256 spp in passes of 16, adaptive_threshold 0.05, 0.1, 0.25 and 0.5, with
           settings.despike off and on (the check alone differs: the frame is the plain divide of the raw sums both times — the despiked run's tiles are
           divided here, not through await_()).  Mean spp and RMSE against a 2,048 spp frame of another seed, beside the uniform 256 spp frame's.
tile_errors  Why that table moves or does not: the same scene and size at 16, 64 and 256 spp, rmd_tile_error (floor 1e-3) of all 2,040 tiles on the raw sums
           and on the despiked ones — at the starting values, at k 0 / ratio 1, at rank 0 and at radius 3 —: the pixels replaced, the tiles whose error
           changed, and the tiles at or below each of the four thresholds before and after.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

LUMA = (0.2126, 0.7152, 0.0722)


def rmse(a, b):
    import numpy as np

    return float(np.sqrt(np.mean((a - b) ** 2)))


def render_sums(ctx, scene, W, H, spp, seed):
    """(S, Q) of a whole-frame render at `spp` samples, one rect."""
    from raymond_amd import render, scenes
    from raymond_amd.scene import Settings, generate_tiles

    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=seed)
    ds, fb, fb_sq = render.DeviceScene(ctx, scene), render.Framebuffer(ctx, W, H), render.Framebuffer(ctx, W, H)
    try:
        render.render_tiles(ctx, ds, st.camera_settings, st, generate_tiles(W, H, (32, 32)), fb, framebuffer_sq=fb_sq)
        return fb.download(), fb_sq.download()
    finally:
        fb.close(), fb_sq.close(), ds.close()


def quality(a):
    import numpy as np

    from raymond_amd import render, scenes

    W, H = 256, 144
    rects = [(0, 0, W, H)]
    result = {"width": W, "height": H, "bounces": 5, "reference_spp": 2048, "despike": dict(radius=2, rank=2, k=6.0, ratio=2.0, floor=0.0), "frames": {}}
    with render.Context(0) as ctx:
        for name, scene in (("reflective_spheres", scenes.reflective_spheres()), ("gold_dragon_standin", scenes.gold_dragon_standin())):
            truth = render_sums(ctx, scene, W, H, 2048, scenes.SEED + 1)[0] / 2048.0
            for spp in (16, 64):
                S, Q = render_sums(ctx, scene, W, H, spp, scenes.SEED)
                dS, dQ, replaced = render.despike_arrays(ctx, S, Q, rects, [spp])
                row = {"replaced": int(replaced.sum()), "replaced_share": float(replaced.sum()) / (W * H),
                       "mean_luminance": float(((S / spp) * LUMA).sum(axis=2).mean()), "mean_luminance_removed": float((((S - dS) / spp) * LUMA).sum(axis=2).mean()),
                       "truth_mean_luminance": float((truth * LUMA).sum(axis=2).mean())}
                for tag, s, q in (("raw", S, Q), ("despiked", dS, dQ)):
                    row["rmse_mean_" + tag] = rmse(s / spp, truth)
                    row["rmse_denoise_" + tag] = rmse(render.denoise_arrays(ctx, s, q, rects, [spp]), truth)
                    row["rmse_atrous_" + tag] = rmse(render.denoise_atrous_arrays(ctx, s, q, None, None, rects, [spp]), truth)
                result["frames"]["%s %d spp" % (name, spp)] = row
                print(name, spp, json.dumps(row), flush=True)
    return result


def adaptive(a):
    import numpy as np

    from raymond_amd import render, scenes
    from raymond_amd.scene import Settings

    W, H = 1920, 1080
    scene = scenes.reflective_spheres()
    result = {"width": W, "height": H, "bounces": 5, "max_spp": 256, "pass": 16, "reference_spp": 2048, "rows": {}}
    with render.Context(0) as ctx:
        truth = render_sums(ctx, scene, W, H, 2048, scenes.SEED + 1)[0] / 2048.0
        result["uniform_256_rmse"] = rmse(render_sums(ctx, scene, W, H, 256, scenes.SEED)[0] / 256.0, truth)
    print("uniform 256 spp: RMSE %.6f" % result["uniform_256_rmse"], flush=True)
    for threshold in (0.05, 0.1, 0.25, 0.5):
        for on in (False, True):
            st = Settings(scenes.camera(W, H), sample_count=256, bounce_limit=5, seed=scenes.SEED, samples_per_iteration=16, adaptive_threshold=threshold,
                          progress_tiles=False, despike=on)
            handle = render.render_tiled(scene, st)
            frame, samples, early = np.zeros((H, W, 3)), 0, 0
            for m in handle._messages:
                if m.kind == "TileFinished":
                    t = m.tile
                    frame[t.top : t.top + t.height, t.left : t.left + t.width] = t.data / float(t.sample_count)  # the raw sums, both times
                    samples += t.sample_count * t.width * t.height
                    early += t.sample_count < 256
            row = {"mean_spp": samples / float(W * H), "tiles_stopped_early": int(early), "rmse": rmse(frame, truth)}
            result["rows"]["threshold %g despike %s" % (threshold, "on" if on else "off")] = row
            print("threshold %g despike %s:" % (threshold, "on" if on else "off"), json.dumps(row), flush=True)
    return result


def tile_errors(a):
    import numpy as np

    from raymond_amd import render, scenes
    from raymond_amd.scene import Settings, generate_tiles

    W, H = 1920, 1080
    tiles = generate_tiles(W, H, (32, 32))
    result = {"width": W, "height": H, "tiles": len(tiles), "floor": 1e-3, "rows": {}}
    with render.Context(0) as ctx:
        ds, fb, fb_sq = render.DeviceScene(ctx, scenes.reflective_spheres()), render.Framebuffer(ctx, W, H), render.Framebuffer(ctx, W, H)
        try:
            done = 0
            for spp in (16, 64, 256):
                st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=scenes.SEED)
                render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fb, done, spp - done, framebuffer_sq=fb_sq)  # (the samples [done, spp) on top)
                done = spp
                raw = render.tile_error(ctx, fb, fb_sq, spp, 1e-3, tiles)
                for name, params in (("starting values", {}), ("k 0 ratio 1", dict(k=0.0, ratio=1.0)), ("rank 0", dict(rank=0)), ("radius 3 rank 2", dict(radius=3))):
                    cS, cQ, replaced = render.despike(ctx, fb, fb_sq, tiles, [spp] * len(tiles), **params)
                    try:
                        clean = render.tile_error(ctx, cS, cQ, spp, 1e-3, tiles)
                    finally:
                        cS.close(), cQ.close()
                    row = {"replaced": int(replaced.sum()), "tiles_with_a_spike": int((replaced > 0).sum()), "tiles_whose_error_changed": int((raw != clean).sum()),
                           "tiles_whose_error_fell": int((clean < raw).sum()), "tiles_whose_error_rose": int((clean > raw).sum()),
                           "median_error_raw": float(np.median(raw)), "median_error_despiked": float(np.median(clean))}
                    for t in (0.05, 0.1, 0.25, 0.5):
                        row["at_or_below_%g_raw" % t] = int((raw <= t).sum())
                        row["at_or_below_%g_despiked" % t] = int((clean <= t).sum())
                    result["rows"]["%d spp, %s" % (spp, name)] = row
                    print(spp, name, json.dumps(row), flush=True)
        finally:
            fb.close(), fb_sq.close(), ds.close()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["quality", "adaptive", "tile_errors"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = {"quality": quality, "adaptive": adaptive, "tile_errors": tile_errors}[a.what](a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
