#!/usr/bin/env python3
"""What rmd_denoise_dual_region costs by the size of its region, at 1920x1080 (one GPU, one call):

    python tools/region_time.py [--runs 9] [--out profiles/r11_region/region_time.json]

ReflectiveSpheres, 16 + 16 samples in the two halves, r = 10, f = 3, the 2,040 tiles of 32 x 32 as the rects.  rmd_denoise_dual, and
rmd_denoise_dual_region over: all 2,040 tiles, a checkerboard half of them, a contiguous quarter (the frame's top left), a random 25 %, 10 % and
1 % (numpy's default_rng(0)), and one tile — alternated, `runs` times each after a warm-up of each.  Every call is the WHOLE call, its scratch
allocation and copies included, bracketed by HIP events recorded on the context's own stream; medians and spreads are reported.

    --once NAME          one warm-up and one call of the named set, nothing else: what a `rocprofv3 --kernel-trace --stats` run wraps
    --full-only          rmd_denoise_dual alone (no region symbol is touched): with --package-root, the same measurement on another tree
    --package-root DIR   import raymond_amd from DIR instead of this file's repository
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

_ap = argparse.ArgumentParser()
_ap.add_argument("--runs", type=int, default=9)
_ap.add_argument("--out", default=None)
_ap.add_argument("--once", default=None)
_ap.add_argument("--full-only", action="store_true")
_ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ARGS = _ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.package_root))
from raymond_amd import render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

from denoise_time import hip  # noqa: E402  (tools/ is this script's directory)


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_pct": 100.0 * (max(v) - min(v)) / min(v), "runs_ms": v}


def region_sets(W, H, tiles):
    cols = (W + 31) // 32
    rng = np.random.default_rng(0)
    sets = {"all_tiles": list(tiles),
            "checkerboard_half": [t for t in tiles if ((t[0] // 32) + (t[1] // 32)) % 2 == 0],
            "contiguous_quarter": [t for t in tiles if t[0] // 32 < cols // 2 and t[1] < 32 * 17]}
    for pct in (25, 10, 1):
        pick = sorted(rng.choice(len(tiles), size=max(1, round(len(tiles) * pct / 100.0)), replace=False))
        sets["random_%d_pct" % pct] = [tiles[i] for i in pick]
    sets["one_tile"] = [tiles[len(tiles) // 2 + cols // 2]]
    return sets


def main():
    a = ARGS
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
    n16 = [16] * len(tiles)
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(5)]  # A, A_sq, B, B_sq, out
    err = render.ErrorImage(ctx, W, H)
    result = {"width": W, "height": H, "runs": a.runs, "radius": 10, "patch_radius": 3, "samples_per_half": 16, "tiles": len(tiles),
              "package_root": os.path.basename(os.path.abspath(a.package_root))}
    try:
        ds = render.DeviceScene(ctx, scenes.reflective_spheres())
        try:
            render.render_tiles(ctx, ds, cam, st, tiles, fbs[0], 0, 16, framebuffer_sq=fbs[1])
            render.render_tiles(ctx, ds, cam, st, tiles, fbs[2], 16, 16, framebuffer_sq=fbs[3])
        finally:
            ds.close()
        fns = {"rmd_denoise_dual": lambda: render.denoise_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), tiles, n16, n16, fbs[4], err)}
        if not a.full_only:
            sets = region_sets(W, H, tiles)
            area = float(W * H)
            result["regions"] = {n: {"tiles": len(r), "pixel_fraction": sum(w * h for (_, _, w, h) in r) / area} for n, r in sets.items()}
            for name, region in sets.items():
                fns["region_" + name] = (lambda region=region: render.denoise_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), tiles, n16, n16, fbs[4], err,
                                                                                    region=region))
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
    finally:
        for b in fbs + [err]:
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
