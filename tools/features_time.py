#!/usr/bin/env python3
"""What the first-hit feature pass and the guided filter cost at 1920x1080 (one GPU, one call):

    python tools/features_time.py [--runs 9] [--out profiles/r09_features/features_time.json] [--rocprof-child]

1. ReflectiveSpheres and the benchmark mesh scene (GoldDragon stand-in), 16 spp, 32 x 32 tiles: rmd_render_features (with squares) against
   
   rmd_render_tiles_moments of the same tiles and samples at the scene's own 5 bounces, alternated, `runs` times each after a warm-up of each.
2. rmd_denoise_guided against rmd_denoise at r = 10, f = 3 on the spheres frame's sums, alternated likewise.
Every call is bracketed by HIP events recorded on the context's own stream (rmd_context_create_on_stream); medians and spreads are reported.
--rocprof-child runs the same calls without the bracketing, for a separate `rocprofv3 --kernel-trace --stats` run.
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
    ap.add_argument("--rocprof-child", action="store_true")
    a = ap.parse_args()
    W, H, spp = 1920, 1080, 16
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
                if a.rocprof_child:
                    fns[name]()
                else:
                    ms[name].append(timed(fns[name]))
        return ms

    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=scenes.SEED)
    cam = st.camera_settings
    tiles = generate_tiles(W, H, (32, 32))
    result = {"width": W, "height": H, "spp": spp, "runs": a.runs, "feature_pass": {}, "filter": {}}
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(3)]
    fts = [render.FeatureBuffer(ctx, W, H) for _ in range(2)]
    try:
        for name, scene in (("gold_dragon_standin", scenes.gold_dragon_standin()), ("reflective_spheres", scenes.reflective_spheres())):
            ds = render.DeviceScene(ctx, scene)
            try:
                def moments():
                    render.render_tiles(ctx, ds, cam, st, tiles, fbs[0], 0, spp, framebuffer_sq=fbs[1])

                def features():
                    render.render_features(ctx, ds, cam, st, tiles, fts[0], 0, spp, features_sq=fts[1])

                ms = alternate({"moments_render": moments, "feature_pass": features})
                if not a.rocprof_child:
                    rec = {k: stats(v) for k, v in ms.items()}
                    rec["feature_over_moments_median"] = rec["feature_pass"]["median_ms"] / rec["moments_render"]["median_ms"]
                    result["feature_pass"][name] = rec
                    print(name, json.dumps(rec), flush=True)
                for b in fbs[:2] + fts:  # (the timed calls went on adding to the sums: start again, so that the last scene's 16 spp are what the filter gets)
                    b.zero()
                moments(), features()
            finally:
                ds.close()
        # the buffers now hold the spheres frame's sums and features
        rect, count = [(0, 0, W, H)], [spp]
        ms = alternate({"rmd_denoise": lambda: render.denoise(ctx, fbs[0], fbs[1], rect, count, fbs[2]),
                        "rmd_denoise_guided": lambda: render.denoise_guided(ctx, fbs[0], fbs[1], fts[0], fts[1], rect, count, fbs[2])})
        if not a.rocprof_child:
            rec = {k: stats(v) for k, v in ms.items()}
            rec["guided_over_unguided_median"] = rec["rmd_denoise_guided"]["median_ms"] / rec["rmd_denoise"]["median_ms"]
            result["filter"] = rec
            print("filter", json.dumps(rec), flush=True)
    finally:
        for b in fbs + fts:
            b.close()
        ctx.close()
        for e in ev:
            H_.hipEventDestroy(e)
        H_.hipStreamDestroy(stream)
    if a.rocprof_child:
        print("rocprof child done")
        return
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
