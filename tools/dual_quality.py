#!/usr/bin/env python3
"""What the dual-buffer filter delivers and how well its error estimate ranks tiles (one GPU):

    python tools/dual_quality.py [--out profiles/r10_dual/dual_quality.json] [--ref-spp 2048]

For ReflectiveSpheres and the small GoldDragon stand-in (n = 24) at 256x144, 5 bounces, 32 x 32 tiles, passes of 8 samples, against a --ref-spp
frame of seed + 1 (whose own noise is part of every RMSE):
  levels    at 16, 32, 64 and 128 spp: the RMSE of rmd_denoise on the samples in one buffer and of rmd_denoise_dual on the same samples in two
            halves; Spearman's rank correlation, over the tiles, of rmd_tile_error_dual with the per-tile RMS error of the dual frame, the
            median of estimate / true error, and the same correlation for rmd_tile_error against rmd_denoise's per-tile error;
  adaptive  render_tiled with adaptive_denoised_threshold at the median and at the 70 % quantile of the 32 spp estimate, at most 128 spp, no
            check below 32: mean spp and RMSE, beside uniform rmd_denoise and rmd_denoise_dual frames at the mean spp rounded up to 16.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

W, H, BOUNCES, SPI = 256, 144, 5, 8


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def ranks(x):
    x = np.asarray(x, dtype=np.float64)
    order = np.argsort(x, kind="stable")
    r = np.empty(len(x))
    i = 0
    while i < len(x):
        j = i
        while j + 1 < len(x) and x[order[j + 1]] == x[order[i]]:
            j += 1
        r[order[i : j + 1]] = (i + j) / 2.0 + 1.0
        i = j + 1
    return r


def spearman(a, b):
    return float(np.corrcoef(ranks(a), ranks(b))[0, 1])


def tile_rms(img, ref, tiles):
    return np.array([math.sqrt(np.mean((img[t : t + h, l : l + w] - ref[t : t + h, l : l + w]) ** 2)) for (l, t, w, h) in tiles])


def moments(ctx, ds, spp, seed):
    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=BOUNCES, seed=seed)
    fb, fb_sq = render.Framebuffer(ctx, W, H), render.Framebuffer(ctx, W, H)
    try:
        render.render_tiles(ctx, ds, st.camera_settings, st, generate_tiles(W, H, (32, 32)), fb, 0, spp, framebuffer_sq=fb_sq)
        return fb, fb_sq, fb.download(), fb_sq.download()
    except Exception:
        fb.close(), fb_sq.close()
        raise


def dual_settings(spp, **kw):
    return Settings(scenes.camera(W, H), sample_count=spp, tile_size=(32, 32), bounce_limit=BOUNCES, seed=scenes.SEED, samples_per_iteration=SPI, denoise=True,
                    denoise_dual=True, **kw)


def finished(handle):
    handle.async_await()
    return [m.tile for m in handle._messages if m.kind == "TileFinished"]


def dual_frame(ctx, tiles_done, tiles):
    """rmd_denoise_dual over finished dual tiles -> (frame, per-tile estimate over `tiles`)."""
    halves = [np.zeros((H, W, 3)) for _ in range(4)]
    for t in tiles_done:
        for dst, src in zip(halves, (t.data_a, t.data_sq_a, t.data_b, t.data_sq_b)):
            dst[t.top : t.top + t.height, t.left : t.left + t.width] = src
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(5)]
    err = render.ErrorImage(ctx, W, H)
    try:
        for fb, arr in zip(fbs, halves):
            fb.upload(arr)
        rects = [(t.left, t.top, t.width, t.height) for t in tiles_done]
        render.denoise_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), rects, [t.count_a for t in tiles_done], [t.count_b for t in tiles_done], fbs[4], err)
        return fbs[4].download(), render.tile_error_dual(ctx, err, tiles)
    finally:
        for b in fbs + [err]:
            b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ref-spp", type=int, default=2048)
    a = ap.parse_args()
    tiles = generate_tiles(W, H, (32, 32))
    out = {"width": W, "height": H, "bounces": BOUNCES, "samples_per_iteration": SPI, "ref_spp": a.ref_spp, "scenes": {}}
    with render.Context(0) as ctx:
        for name, scene in (("reflective_spheres", scenes.reflective_spheres()), ("gold_dragon_standin_n24", scenes.gold_dragon_standin(n=24))):
            ds = render.DeviceScene(ctx, scene)
            try:
                fb, fb_sq, S_ref, _ = moments(ctx, ds, a.ref_spp, scenes.SEED + 1)
                fb.close(), fb_sq.close()
                ref = S_ref / a.ref_spp
                rec = {"levels": [], "adaptive": []}
                estimate32 = None
                for spp in (16, 32, 64, 128):
                    fb, fb_sq, S, Q = moments(ctx, ds, spp, scenes.SEED)
                    try:
                        raw_rule = render.tile_error(ctx, fb, fb_sq, spp, 1e-3, tiles)
                    finally:
                        fb.close(), fb_sq.close()
                    single = render.denoise_arrays(ctx, S, Q, [(0, 0, W, H)], [spp])
                    dual, estimate = dual_frame(ctx, finished(render.render_tiled(scene, dual_settings(spp))), tiles)
                    true = tile_rms(dual, ref, tiles)
                    if spp == 32:
                        estimate32 = estimate
                    rec["levels"].append({"spp": spp, "rmse_noisy": rmse(S / spp, ref), "rmse_rmd_denoise": rmse(single, ref), "rmse_rmd_denoise_dual": rmse(dual, ref),
                                          "spearman_dual_estimate": spearman(estimate, true), "median_estimate_over_true": float(np.median(estimate / true)),
                                          "spearman_raw_rule": spearman(raw_rule, tile_rms(single, ref, tiles))})
                    print(name, json.dumps(rec["levels"][-1]), flush=True)
                for label, thr in (("median", float(np.median(estimate32))), ("quantile_70", float(np.quantile(estimate32, 0.7)))):
                    handle = render.render_tiled(scene, dual_settings(128, adaptive_denoised_threshold=thr, adaptive_min_samples=32))
                    done = finished(handle)
                    mean_spp = sum(t.sample_count * t.width * t.height for t in done) / float(W * H)
                    frame = handle.await_()
                    n = int(math.ceil(mean_spp / 16.0)) * 16
                    fb, fb_sq, S, Q = moments(ctx, ds, n, scenes.SEED)
                    fb.close(), fb_sq.close()
                    single = render.denoise_arrays(ctx, S, Q, [(0, 0, W, H)], [n])
                    dual, _ = dual_frame(ctx, finished(render.render_tiled(scene, dual_settings(n))), tiles)
                    rec["adaptive"].append({"threshold": label, "threshold_value": thr, "mean_spp": mean_spp, "tiles_early": sum(t.sample_count < 128 for t in done),
                                            "tiles": len(done), "rmse_adaptive": rmse(frame, ref), "uniform_spp": n, "rmse_uniform_rmd_denoise": rmse(single, ref),
                                            "rmse_uniform_rmd_denoise_dual": rmse(dual, ref)})
                    print(name, json.dumps(rec["adaptive"][-1]), flush=True)
                out["scenes"][name] = rec
            finally:
                ds.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
