#!/usr/bin/env python3
"""What the a-trous filter costs beside the non-local means filters, at 1920x1080 (one GPU, one call):

    python tools/atrous_time.py [--runs 9] [--out profiles/r14_atrous/atrous_time.json]

ReflectiveSpheres, 16 samples, the first-hit features of the same samples, the 2,040 tiles of 32 x 32 as the rects.  rmd_denoise_atrous at 1, 3 and
5 levels (k 3.0, alpha 1; guided: k_f 1.0, tau 1e-2), guided and unguided, alternated in one process with rmd_denoise and rmd_denoise_guided at
their defaults on the same buffers, `runs` times each after a warm-up of each.  Every call is the WHOLE call, its scratch allocation and copies
included, bracketed by HIP events recorded on the context's own stream; medians and spreads are reported.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

from denoise_time import hip  # noqa: E402  (tools/ is this script's directory)
from dual_guided_time import stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=None)
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

    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=scenes.SEED)
    cam = st.camera_settings
    tiles = generate_tiles(W, H, (32, 32))
    counts = [spp] * len(tiles)
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(3)]  # S, Q, out
    feat = [render.FeatureBuffer(ctx, W, H) for _ in range(2)]
    result = {"width": W, "height": H, "runs": a.runs, "samples": spp, "tiles": len(tiles), "atrous_k": 3.0, "alpha": 1.0, "k_f": 1.0, "tau": 1e-2,
              "nlm": {"radius": 10, "patch_radius": 3, "k": 0.45}}
    try:
        ds = render.DeviceScene(ctx, scenes.reflective_spheres())
        try:
            render.render_tiles(ctx, ds, cam, st, tiles, fbs[0], 0, spp, framebuffer_sq=fbs[1])
            render.render_features(ctx, ds, cam, st, tiles, feat[0], 0, spp, features_sq=feat[1])
        finally:
            ds.close()
        guide = dict(features=feat[0], features_sq=feat[1])
        fns = {"rmd_denoise": lambda: render.denoise(ctx, fbs[0], fbs[1], tiles, counts, fbs[2]),
               "rmd_denoise_guided": lambda: render.denoise_guided(ctx, fbs[0], fbs[1], feat[0], feat[1], tiles, counts, fbs[2])}
        for levels in (1, 3, 5):
            fns["atrous_%d_unguided" % levels] = lambda levels=levels: render.denoise_atrous(ctx, fbs[0], fbs[1], tiles, counts, fbs[2], levels=levels)
            fns["atrous_%d_guided" % levels] = lambda levels=levels: render.denoise_atrous(ctx, fbs[0], fbs[1], tiles, counts, fbs[2], levels=levels, **guide)
        for fn in fns.values():
            fn()  # warm-up: code objects, the LDS attribute
        ms = {n: [] for n in fns}
        for r in range(a.runs):
            for name in (list(fns) if r % 2 == 0 else list(reversed(fns))):  # alternated: drift falls on all alike
                ms[name].append(timed(fns[name]))
        result["calls"] = {k: stats(v) for k, v in ms.items()}
        for k, v in result["calls"].items():
            print(k, "%.3f ms (min %.3f, max %.3f)" % (v["median_ms"], v["min_ms"], v["max_ms"]), flush=True)
        med = {k: v["median_ms"] for k, v in result["calls"].items()}
        result["nlm_over_atrous_5"] = {"unguided": med["rmd_denoise"] / med["atrous_5_unguided"], "guided": med["rmd_denoise_guided"] / med["atrous_5_guided"]}
    finally:
        for b in fbs + feat:
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
