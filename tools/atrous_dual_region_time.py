#!/usr/bin/env python3
"""What rmd_denoise_atrous_dual_region costs by the size and the shape of its region, at 1920x1080 (one GPU, one call):

    python tools/atrous_dual_region_time.py [--runs 9] [--out profiles/r16_atrous_dual_region/region_time.json]

ReflectiveSpheres, 8 + 8 samples in the two halves, the first-hit features of the same 16 samples, the 2,040 tiles of 32 x 32 as the rects, k 3.0,
alpha 1 (guided: k_f 1.0, tau 1e-2).  At 3 and at 5 levels, unguided and guided: rmd_denoise_atrous_dual, and rmd_denoise_atrous_dual_region over all
2,040 tiles, a checkerboard half of them, a contiguous quarter (the frame's top left), a random 25 %, 10 % and 1 % (numpy's default_rng(0)), and
one tile — alternated, `runs` times each after a warm-up of each.  Every call is the WHOLE call, its copies (and the whole-frame call's scratch
allocation) included, bracketed by HIP events recorded on the context's own stream; medians and spreads are reported.  One pass of 8 samples over
every tile is timed the same way: with it, per region set, the check's cost over the cost of the two passes between checks over the same tiles.

    --once NAME     one warm-up and one call of the named entry (as printed), nothing else: what a `rocprofv3 --kernel-trace --stats` run wraps
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


def region_sets(W, H, tiles):
    """tools/region_time.py's sets (that script reads its arguments when it is imported, so they are restated)."""
    import numpy as np

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
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", default=None)
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
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(7)]  # A, A_sq, B, B_sq, out, and two for the timed pass
    err = render.ErrorImage(ctx, W, H)
    feat = [render.FeatureBuffer(ctx, W, H) for _ in range(2)]
    sets = region_sets(W, H, tiles)
    area = float(W * H)
    result = {"width": W, "height": H, "runs": a.runs, "samples_per_half": half, "tiles": len(tiles), "levels": [3, 5], "atrous_k": 3.0, "alpha": 1.0, "k_f": 1.0,
              "tau": 1e-2, "regions": {n: {"tiles": len(r), "pixel_fraction": sum(w * h for (_, _, w, h) in r) / area} for n, r in sets.items()}}
    ds = render.DeviceScene(ctx, scenes.reflective_spheres())
    try:
        render.render_tiles(ctx, ds, cam, st, tiles, fbs[0], 0, half, framebuffer_sq=fbs[1])
        render.render_tiles(ctx, ds, cam, st, tiles, fbs[2], half, half, framebuffer_sq=fbs[3])
        render.render_features(ctx, ds, cam, st, tiles, feat[0], 0, 2 * half, features_sq=feat[1])
        A, B = (fbs[0], fbs[1]), (fbs[2], fbs[3])
        fns = {"pass_8_samples": lambda: render.render_tiles(ctx, ds, cam, st, tiles, fbs[5], 16, 8, framebuffer_sq=fbs[6])}
        for levels in (3, 5):
            for mode, guide in (("unguided", {}), ("guided", dict(features=feat[0], features_sq=feat[1], counts_f=n_both))):
                tag = "levels_%d_%s_" % (levels, mode)
                fns[tag + "whole_frame"] = (lambda levels=levels, guide=guide: render.denoise_atrous_dual(ctx, A, B, tiles, n_half, n_half, fbs[4], err, levels=levels, **guide))
                for name, region in sets.items():
                    fns[tag + "region_" + name] = (lambda levels=levels, guide=guide, region=region: render.denoise_atrous_dual(
                        ctx, A, B, tiles, n_half, n_half, fbs[4], err, levels=levels, region=region, **guide))
        if a.once:
            fns[a.once]()  # warm-up: code objects, the context's scratch
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
            # per region set: the call over the whole-frame call, and over the two 8-sample passes between checks over the same tiles (below 1 the check
            # is the smaller part)
            result["region_over_whole_frame"] = {k: med[k] / med[k[: k.index("region_")] + "whole_frame"] for k in med if "region_" in k}
            result["check_over_two_passes_spheres_spi_8"] = {
                k: med[k] / (2.0 * med["pass_8_samples"] * result["regions"][k[k.index("region_") + len("region_"):]]["pixel_fraction"]) for k in med if "region_" in k}
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


if __name__ == "__main__":
    main()
