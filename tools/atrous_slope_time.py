#!/usr/bin/env python3
"""What the feature-slope term costs the guided a-trous filters, at 1920x1080 (one GPU, one call):

    python tools/atrous_slope_time.py [--runs 9] [--out profiles/r21_atrous_slope/atrous_slope_time.json]

ReflectiveSpheres, 8 + 8 samples, the first-hit features of the same 16 samples, the 2,040 tiles of 32 x 32 as the rects; k 3.0, alpha 1, k_f 1.0,
tau 1e-2; 3 and 5 levels.  Per level count, the call without the suffix (guided) against its _slope call at slope 3, alternated in one process, `runs`
times each after a warm-up of each:
    rmd_denoise_atrous on the merged sums, rmd_denoise_atrous_dual on the two halves, and rmd_denoise_atrous_dual_region over one tile, a contiguous
    quarter and a random quarter of the tiles (tools/atrous_dual_region_time.py's sets).
Every call is the WHOLE call, its scratch and copies included, bracketed by HIP events on the context's own stream; medians and spreads are reported,
and per pair the difference of the medians.  The whole-frame dual call's difference holds one feature_slope_kernel pass over the frame (and seven loads a
pixel a level): a one-tile region call whose difference reaches it would be making its slopes over the whole frame.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

from atrous_dual_region_time import region_sets  # noqa: E402  (tools/ is this script's directory)
from denoise_time import hip  # noqa: E402
from dual_guided_time import stats  # noqa: E402

SLOPE = 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H, half = 1920, 1080, 8
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

    st = Settings(scenes.camera(W, H), sample_count=2 * half, bounce_limit=5, seed=scenes.SEED)
    cam = st.camera_settings
    tiles = generate_tiles(W, H, (32, 32))
    n_half, n_both = [half] * len(tiles), [2 * half] * len(tiles)
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(7)]  # A, A_sq, B, B_sq, out, and the merged sums and squares
    err = render.ErrorImage(ctx, W, H)
    feat = [render.FeatureBuffer(ctx, W, H) for _ in range(2)]
    sets = {k: v for k, v in region_sets(W, H, tiles).items() if k in ("one_tile", "contiguous_quarter", "random_25_pct")}
    result = {"width": W, "height": H, "runs": a.runs, "samples_per_half": half, "tiles": len(tiles), "levels": [3, 5], "atrous_k": 3.0, "alpha": 1.0, "k_f": 1.0,
              "tau": 1e-2, "slope": SLOPE, "regions": {n: len(r) for n, r in sets.items()}}
    ds = render.DeviceScene(ctx, scenes.reflective_spheres())
    try:
        render.render_tiles(ctx, ds, cam, st, tiles, fbs[0], 0, half, framebuffer_sq=fbs[1])
        render.render_tiles(ctx, ds, cam, st, tiles, fbs[2], half, half, framebuffer_sq=fbs[3])
        render.render_tiles(ctx, ds, cam, st, tiles, fbs[5], 0, 2 * half, framebuffer_sq=fbs[6])
        render.render_features(ctx, ds, cam, st, tiles, feat[0], 0, 2 * half, features_sq=feat[1])
        A, B = (fbs[0], fbs[1]), (fbs[2], fbs[3])
        g1 = dict(features=feat[0], features_sq=feat[1])
        g2 = dict(g1, counts_f=n_both)
        fns = {}
        for levels in (3, 5):
            for tag, slope in (("guided", {}), ("slope", dict(slope=SLOPE))):
                head = "levels_%d_" % levels
                fns[head + "single_" + tag] = lambda levels=levels, slope=slope: render.denoise_atrous(ctx, fbs[5], fbs[6], tiles, n_both, fbs[4], levels=levels, **g1, **slope)
                fns[head + "dual_" + tag] = lambda levels=levels, slope=slope: render.denoise_atrous_dual(ctx, A, B, tiles, n_half, n_half, fbs[4], err, levels=levels, **g2, **slope)
                for name, region in sets.items():
                    fns[head + "region_" + name + "_" + tag] = (lambda levels=levels, slope=slope, region=region: render.denoise_atrous_dual(
                        ctx, A, B, tiles, n_half, n_half, fbs[4], err, levels=levels, region=region, **g2, **slope))
        for fn in fns.values():
            fn()  # warm-up: code objects, the context's scratch
        ms = {n: [] for n in fns}
        for r in range(a.runs):
            for name in (list(fns) if r % 2 == 0 else list(reversed(fns))):  # alternated: drift falls on all alike
                ms[name].append(timed(fns[name]))
        result["calls"] = {k: stats(v) for k, v in ms.items()}
        for k, v in result["calls"].items():
            print(k, "%.3f ms (min %.3f, max %.3f)" % (v["median_ms"], v["min_ms"], v["max_ms"]), flush=True)
        med = {k: v["median_ms"] for k, v in result["calls"].items()}
        result["slope_minus_guided_ms"] = {k[: -len("_slope")]: med[k] - med[k[: -len("_slope")] + "_guided"] for k in med if k.endswith("_slope")}
    finally:
        ds.close()
        for b in fbs + [err] + feat:
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
            f.write("\n")


if __name__ == "__main__":
    main()
