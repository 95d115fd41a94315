#!/usr/bin/env python3
"""What rmd_despike_dual does to a dual-buffer frame's error, and to adaptive sampling, on one GPU:

    python tools/despike_dual_quality.py quality  [--out profiles/r28_despike_dual/quality.json]
    python tools/despike_dual_quality.py adaptive [--out profiles/r28_despike_dual/adaptive.json]

quality    256 x 144, 16 and 64 spp (half A the first half of the samples, half B the second), 5 bounces, scenes.firefly_spheres() and the two bundled
           scenes, rmd_despike_dual at the starting values (radius 2, rank 2, k 6, ratio 2, floor 0).  RMSE of rmd_denoise_dual's (radius 10, patch 3,
           k 0.45) and rmd_denoise_atrous_dual's (5 levels, k 3) frames with the stage off and on, against a 2,048 spp frame of another seed; the pixels
           replaced and the mean luminance removed.  The firefly scene's reference frame has fireflies of its own: a second column gives the RMSE over the
           pixels the reference's own rmd_despike (at 2,048 samples) leaves alone.
adaptive   firefly_spheres at 256 x 144 in 16 x 16 tiles, up to 128 spp in passes of 8, 5 bounces.  The dual loop (rmd_denoise_dual radius 5, patch 2) with
           adaptive_denoised_threshold 0.01, 0.02 and 0.04 from 32 samples on, despike_dual off and on: tiles stopped early, mean spp, the RMSE of await_()'s
           frame against the 2,048 spp reference (whole frame, and over the pixels the reference's own rmd_despike leaves alone).  And the single-buffer
           loop on the same scene: adaptive_threshold 0.1, 0.25 and 0.5 with despike off and on, the frame the plain divide of the raw sums both times.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

LUMA = (0.2126, 0.7152, 0.0722)
W, H = 256, 144


def reference(ctx, scene):
    """(the 2,048 spp means of another seed, the mask of the pixels its own rmd_despike leaves alone)"""
    import numpy as np

    from despike_quality import render_sums
    from raymond_amd import render, scenes

    S, Q = render_sums(ctx, scene, W, H, 2048, scenes.SEED + 1)
    dS, dQ, replaced = render.despike_arrays(ctx, S, Q, [(0, 0, W, H)], [2048])
    alone = (S.view(np.uint64) == dS.view(np.uint64)).all(axis=2) & (Q.view(np.uint64) == dQ.view(np.uint64)).all(axis=2)
    return S / 2048.0, alone, int(replaced.sum())


def rmse2(frame, truth, alone):
    import numpy as np

    d = (frame - truth) ** 2
    return float(np.sqrt(np.mean(d))), float(np.sqrt(np.mean(d[alone])))


def render_halves(ctx, scene, spp, seed):
    from raymond_amd import render, scenes
    from raymond_amd.scene import Settings, generate_tiles

    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=seed)
    ds = render.DeviceScene(ctx, scene)
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(4)]
    try:
        tiles = generate_tiles(W, H, (32, 32))
        render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fbs[0], 0, spp // 2, framebuffer_sq=fbs[1])
        render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fbs[2], spp // 2, spp // 2, framebuffer_sq=fbs[3])
        return [fb.download() for fb in fbs]
    finally:
        for fb in fbs:
            fb.close()
        ds.close()


def quality(a):
    from raymond_amd import render, scenes

    rects = [(0, 0, W, H)]
    result = {"width": W, "height": H, "bounces": 5, "reference_spp": 2048, "despike": dict(radius=2, rank=2, k=6.0, ratio=2.0, floor=0.0), "frames": {}}
    with render.Context(0) as ctx:
        for name, scene in (("firefly_spheres", scenes.firefly_spheres()), ("reflective_spheres", scenes.reflective_spheres()),
                            ("gold_dragon_standin", scenes.gold_dragon_standin())):
            truth, alone, own = reference(ctx, scene)
            result["reference %s" % name] = {"pixels_its_own_despike_replaces": own}
            for spp in (16, 64):
                halves = render_halves(ctx, scene, spp, scenes.SEED)
                n = [spp // 2]
                clean = render.despike_dual_arrays(ctx, *halves, rects, n, n)
                removed = ((halves[0] + halves[2]) - (clean[0] + clean[2])) / spp
                row = {"replaced": int(clean[4].sum()), "replaced_share": float(clean[4].sum()) / (W * H), "mean_luminance": float((((halves[0] + halves[2]) / spp) * LUMA).sum(axis=2).mean()),
                       "mean_luminance_removed": float((removed * LUMA).sum(axis=2).mean())}
                for tag, h in (("off", halves), ("on", clean[:4])):
                    row["rmse_dual_" + tag], row["rmse_dual_%s_where_reference_is_clean" % tag] = rmse2(render.denoise_dual_arrays(ctx, *h, rects, n, n)[0], truth, alone)
                    row["rmse_atrous_dual_" + tag], row["rmse_atrous_dual_%s_where_reference_is_clean" % tag] = rmse2(
                        render.denoise_atrous_dual_arrays(ctx, *h, rects, n, n)[0], truth, alone)
                result["frames"]["%s %d spp" % (name, spp)] = row
                print(name, spp, json.dumps(row), flush=True)
    return result


def adaptive(a):
    import numpy as np

    from raymond_amd import render, scenes
    from raymond_amd.scene import Settings

    scene = scenes.firefly_spheres()
    top = 128
    result = {"width": W, "height": H, "bounces": 5, "max_spp": top, "pass": 8, "tile": 16, "reference_spp": 2048, "dual": {}, "single": {}}
    with render.Context(0) as ctx:
        truth, alone, own = reference(ctx, scene)
    result["reference_pixels_its_own_despike_replaces"] = own
    base = dict(sample_count=top, tile_size=(16, 16), bounce_limit=5, seed=scenes.SEED, samples_per_iteration=8, progress_tiles=False)
    for threshold in (0.01, 0.02, 0.04):
        for on in (False, True):
            st = Settings(scenes.camera(W, H), denoise=True, denoise_dual=True, denoise_radius=5, denoise_patch=2, adaptive_denoised_threshold=threshold, adaptive_min_samples=32,
                          despike_dual=on, **base)
            handle = render.render_tiled(scene, st)
            done = [m.tile for m in handle._messages if m.kind == "TileFinished"]
            samples = sum(t.sample_count * t.width * t.height for t in done)
            handle.async_await()
            whole, clean = rmse2(handle.await_(), truth, alone)
            row = {"tiles": len(done), "tiles_stopped_early": sum(1 for t in done if t.sample_count < top), "mean_spp": samples / float(W * H), "rmse": whole,
                   "rmse_where_reference_is_clean": clean}
            result["dual"]["threshold %g despike_dual %s" % (threshold, "on" if on else "off")] = row
            print("dual threshold %g despike_dual %s:" % (threshold, "on" if on else "off"), json.dumps(row), flush=True)
    for threshold in (0.1, 0.25, 0.5):
        for on in (False, True):
            st = Settings(scenes.camera(W, H), adaptive_threshold=threshold, despike=on, **base)
            handle = render.render_tiled(scene, st)
            frame, samples, early, n = np.zeros((H, W, 3)), 0, 0, 0
            for m in handle._messages:
                if m.kind == "TileFinished":
                    t = m.tile
                    frame[t.top : t.top + t.height, t.left : t.left + t.width] = t.data / float(t.sample_count)  # the raw sums, both times
                    samples += t.sample_count * t.width * t.height
                    early += t.sample_count < top
                    n += 1
            whole, clean = rmse2(frame, truth, alone)
            row = {"tiles": n, "tiles_stopped_early": int(early), "mean_spp": samples / float(W * H), "rmse": whole, "rmse_where_reference_is_clean": clean}
            result["single"]["threshold %g despike %s" % (threshold, "on" if on else "off")] = row
            print("single threshold %g despike %s:" % (threshold, "on" if on else "off"), json.dumps(row), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["quality", "adaptive"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = {"quality": quality, "adaptive": adaptive}[a.what](a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
