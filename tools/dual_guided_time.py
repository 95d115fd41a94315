#!/usr/bin/env python3
"""What the feature weight costs in the dual-buffer filter, at 1920x1080 (one GPU, one call):

    python tools/dual_guided_time.py [--runs 9] [--out profiles/r12_dual_guided/dual_guided_time.json]

ReflectiveSpheres, 16 + 16 samples in the two halves, the first-hit features of the same 32 samples, r = 10, f = 3, k_f = 1.0, tau = 1e-2, the
2,040 tiles of 32 x 32 as the rects.  rmd_denoise_dual_guided against rmd_denoise_dual, and the two region forms over all tiles, a random 25 %
(numpy's default_rng(0)) and one tile — alternated, `runs` times each after a warm-up of each.  Every call is the WHOLE call, its scratch
allocation and copies included, bracketed by HIP events recorded on the context's own stream; medians and spreads are reported.

    --once NAME   one warm-up and one call of the named entry, nothing else: what a `rocprofv3 --kernel-trace --stats` run wraps
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

from denoise_time import hip  # noqa: E402  (tools/ is this script's directory)


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_pct": 100.0 * (max(v) - min(v)) / min(v), "runs_ms": v}


def region_sets(W, tiles):
    """tools/region_time.py's all_tiles, random_25_pct and one_tile."""
    pick = sorted(np.random.default_rng(0).choice(len(tiles), size=max(1, round(len(tiles) * 0.25)), replace=False))
    return {"all_tiles": list(tiles), "random_25_pct": [tiles[i] for i in pick], "one_tile": [tiles[len(tiles) // 2 + ((W + 31) // 32) // 2]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", default=None)
    a = ap.parse_args()
    W, H = 1920, 1080
    H_ = hip()
    stream = C.c_void_p()
    assert H_.hipStreamCreate(C.byref(stream)) == 0
    ctx = render.Context(0, stream=stream.value)
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert H_.hipEventCreate(C.byref(e)) == 0

    def timed(fn):
        H_.hipEventRecord(ev[0], stream)
        fn()
        H_.hipEventRecord(ev[1], stream)
        H_.hipEventSynchronize(ev[1])
        f = C.c_float()
        H_.hipEventElapsedTime(C.byref(f), ev[0], ev[1])
        return f.value

    st = Settings(scenes.camera(W, H), sample_count=32, bounce_limit=5, seed=scenes.SEED)
    cam = st.camera_settings
    tiles = generate_tiles(W, H, (32, 32))
    n16, n32 = [16] * len(tiles), [32] * len(tiles)
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(5)]  # A, A_sq, B, B_sq, out
    feat = [render.FeatureBuffer(ctx, W, H) for _ in range(2)]
    err = render.ErrorImage(ctx, W, H)
    result = {"width": W, "height": H, "runs": a.runs, "radius": 10, "patch_radius": 3, "k_f": 1.0, "tau": 1e-2, "samples_per_half": 16, "feature_samples": 32,
              "tiles": len(tiles)}
    try:
        ds = render.DeviceScene(ctx, scenes.reflective_spheres())
        try:
            render.render_tiles(ctx, ds, cam, st, tiles, fbs[0], 0, 16, framebuffer_sq=fbs[1])
            render.render_tiles(ctx, ds, cam, st, tiles, fbs[2], 16, 16, framebuffer_sq=fbs[3])
            render.render_features(ctx, ds, cam, st, tiles, feat[0], 0, 32, features_sq=feat[1])
        finally:
            ds.close()
        sets = region_sets(W, tiles)
        area = float(W * H)
        result["regions"] = {n: {"tiles": len(r), "pixel_fraction": sum(w * h for (_, _, w, h) in r) / area} for n, r in sets.items()}
        guide = dict(features=feat[0], features_sq=feat[1], counts_f=n32, k_f=1.0, tau=1e-2)

        def call(region, guided):
            return lambda: render.denoise_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), tiles, n16, n16, fbs[4], err, region=region, **(guide if guided else {}))

        fns = {"rmd_denoise_dual": call(None, False), "rmd_denoise_dual_guided": call(None, True)}
        for name, region in sets.items():
            fns["region_" + name] = call(region, False)
            fns["guided_region_" + name] = call(region, True)
        if a.once:
            fns[a.once]()  # warm-up: code object, LDS attribute
            result["once"] = {a.once: timed(fns[a.once])}
        else:
            for fn in fns.values():
                fn()  # warm-up
            ms = {n: [] for n in fns}
            for r in range(a.runs):
                for name in (list(fns) if r % 2 == 0 else list(reversed(fns))):  # alternated: drift falls on all alike
                    ms[name].append(timed(fns[name]))
            result["calls"] = {k: stats(v) for k, v in ms.items()}
            for k, v in result["calls"].items():
                print(k, "%.3f ms (min %.3f, max %.3f)" % (v["median_ms"], v["min_ms"], v["max_ms"]), flush=True)
            med = {k: v["median_ms"] for k, v in result["calls"].items()}
            result["guided_over_unguided"] = {"whole_frame": med["rmd_denoise_dual_guided"] / med["rmd_denoise_dual"],
                                              **{n: med["guided_region_" + n] / med["region_" + n] for n in sets}}
    finally:
        for b in fbs + feat + [err]:
            b.close()
        ctx.close()
        for e in ev:
            H_.hipEventDestroy(e)
        H_.hipStreamDestroy(stream)
    print(json.dumps({k: v for k, v in result.items() if k != "calls"}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
