#!/usr/bin/env python3
"""What the dual-buffer filter and one adaptive check cost at 1920x1080 (one GPU, one call):

    python tools/dual_time.py [--runs 9] [--out profiles/r10_dual/dual_time.json]

1. ReflectiveSpheres, 16 spp in passes of 8 (half A: samples 0 .. 7, half B: 8 .. 15), r = 10, f = 3: rmd_denoise_dual (with its error image)
   against rmd_denoise on the sums of the same 16 samples in one buffer, and the whole adaptive check (rmd_denoise_dual + rmd_tile_error_dual
   over the 32 x 32 tiles), alternated, `runs` times each after a warm-up of each.
2. What a check is measured against: one moments pass of 8 and of 64 samples over every tile, for ReflectiveSpheres and the benchmark mesh scene.
Every call is bracketed by HIP events recorded on the context's own stream; medians and spreads are reported.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

from denoise_time import hip  # noqa: E402  (tools/ is this script's directory)


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_pct": 100.0 * (max(v) - min(v)) / min(v), "runs_ms": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=None)
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

    def alternate(fns):
        for fn in fns.values():
            fn()  # warm-up: code objects, LDS attributes, scratch
        ms = {n: [] for n in fns}
        for r in range(a.runs):
            for name in (list(fns) if r % 2 == 0 else list(reversed(fns))):  # alternated: drift falls on both alike
                ms[name].append(timed(fns[name]))
        return {k: stats(v) for k, v in ms.items()}

    st = Settings(scenes.camera(W, H), sample_count=64, bounce_limit=5, seed=scenes.SEED)
    cam = st.camera_settings
    tiles = generate_tiles(W, H, (32, 32))
    result = {"width": W, "height": H, "runs": a.runs, "radius": 10, "patch_radius": 3}
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(8)]  # A, A_sq, B, B_sq, merged, merged_sq, out, pass scratch
    err = render.ErrorImage(ctx, W, H)
    try:
        passes = {}
        for name, scene in (("gold_dragon_standin", scenes.gold_dragon_standin()), ("reflective_spheres", scenes.reflective_spheres())):
            ds = render.DeviceScene(ctx, scene)
            try:
                passes[name] = alternate({"moments_pass_%d" % n: (lambda n=n: render.render_tiles(ctx, ds, cam, st, tiles, fbs[7], 0, n, framebuffer_sq=fbs[6]))
                                          for n in (8, 64)})
                print(name, json.dumps(passes[name]), flush=True)
                if name == "reflective_spheres":
                    render.render_tiles(ctx, ds, cam, st, tiles, fbs[0], 0, 8, framebuffer_sq=fbs[1])
                    render.render_tiles(ctx, ds, cam, st, tiles, fbs[2], 8, 8, framebuffer_sq=fbs[3])
                    render.render_tiles(ctx, ds, cam, st, tiles, fbs[4], 0, 16, framebuffer_sq=fbs[5])
            finally:
                ds.close()
        result["passes"] = passes
        rect = [(0, 0, W, H)]
        n8, n16 = [8] * len(tiles), [16] * len(tiles)

        def check():
            render.denoise_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), tiles, n8, n8, fbs[6], err)
            render.tile_error_dual(ctx, err, tiles)

        rec = alternate({"rmd_denoise": lambda: render.denoise(ctx, fbs[4], fbs[5], tiles, n16, fbs[6]),
                         "rmd_denoise_dual": lambda: render.denoise_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), tiles, n8, n8, fbs[6], err),
                         "adaptive_check": check})
        rec["dual_over_single_median"] = rec["rmd_denoise_dual"]["median_ms"] / rec["rmd_denoise"]["median_ms"]
        result["filter"] = rec
        print("filter", json.dumps(rec), flush=True)
        for name in passes:
            result.setdefault("check_over_pass", {})[name] = {k: rec["adaptive_check"]["median_ms"] / v["median_ms"] for k, v in passes[name].items()}
        print("check_over_pass", json.dumps(result["check_over_pass"]), flush=True)
    finally:
        for b in fbs + [err]:
            b.close()
        ctx.close()
        for e in ev:
            H_.hipEventDestroy(e)
        H_.hipStreamDestroy(stream)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
