#!/usr/bin/env python3
"""What rmd_denoise_atrous_dual costs beside the calls it replaces, at 1920x1080 (one GPU, one call):

    python tools/atrous_dual_time.py [--runs 9] [--out profiles/r15_atrous_dual/atrous_dual_time.json]

ReflectiveSpheres, 8 + 8 samples in the two halves, the first-hit features of the same 16 samples, the 2,040 tiles of 32 x 32 as the rects.
rmd_denoise_atrous_dual at 5 levels (k 3.0, alpha 1; guided: k_f 1.0, tau 1e-2), unguided and guided, alternated in one process with: two
rmd_denoise_atrous calls, one on each half (unguided and guided); rmd_denoise_dual at its defaults; rmd_denoise_dual_region over all tiles —
`runs` times each after a warm-up of each.  Every call is the WHOLE call, its scratch allocation and copies included, bracketed by HIP events
recorded on the context's own stream; medians and spreads are reported.  One pass of 8 and of 64 samples over every tile of the same scene is
timed the same way: with them, the live fraction p above which the check (a constant: the call has no region form) costs less than the two passes
between checks (2 p times a pass over the frame).
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
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(7)]  # A, A_sq, B, B_sq, out, and two for the timed passes
    err = render.ErrorImage(ctx, W, H)
    feat = [render.FeatureBuffer(ctx, W, H) for _ in range(2)]
    result = {"width": W, "height": H, "runs": a.runs, "samples_per_half": half, "tiles": len(tiles), "levels": 5, "atrous_k": 3.0, "alpha": 1.0, "k_f": 1.0,
              "tau": 1e-2, "nlm": {"radius": 10, "patch_radius": 3, "k": 0.45}}
    ds = render.DeviceScene(ctx, scenes.reflective_spheres())
    try:
        render.render_tiles(ctx, ds, cam, st, tiles, fbs[0], 0, half, framebuffer_sq=fbs[1])
        render.render_tiles(ctx, ds, cam, st, tiles, fbs[2], half, half, framebuffer_sq=fbs[3])
        render.render_features(ctx, ds, cam, st, tiles, feat[0], 0, 2 * half, features_sq=feat[1])
        A, B = (fbs[0], fbs[1]), (fbs[2], fbs[3])
        guide = dict(features=feat[0], features_sq=feat[1])

        def two_singles(**kw):
            render.denoise_atrous(ctx, *A, tiles, n_half, fbs[4], **kw)
            render.denoise_atrous(ctx, *B, tiles, n_half, fbs[4], **kw)

        fns = {"atrous_dual_unguided": lambda: render.denoise_atrous_dual(ctx, A, B, tiles, n_half, n_half, fbs[4], err),
               "atrous_dual_guided": lambda: render.denoise_atrous_dual(ctx, A, B, tiles, n_half, n_half, fbs[4], err, counts_f=n_both, **guide),
               "two_atrous_unguided": lambda: two_singles(),
               "two_atrous_guided": lambda: two_singles(**guide),
               "rmd_denoise_dual": lambda: render.denoise_dual(ctx, A, B, tiles, n_half, n_half, fbs[4], err),
               "rmd_denoise_dual_region_all_tiles": lambda: render.denoise_dual(ctx, A, B, tiles, n_half, n_half, fbs[4], err, region=tiles),
               "pass_8_samples": lambda: render.render_tiles(ctx, ds, cam, st, tiles, fbs[5], 16, 8, framebuffer_sq=fbs[6]),
               "pass_64_samples": lambda: render.render_tiles(ctx, ds, cam, st, tiles, fbs[5], 16, 64, framebuffer_sq=fbs[6])}
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
        result["dual_over_two_singles"] = {"unguided": med["atrous_dual_unguided"] / med["two_atrous_unguided"],
                                           "guided": med["atrous_dual_guided"] / med["two_atrous_guided"]}
        result["nlm_dual_over_atrous_dual_unguided"] = med["rmd_denoise_dual"] / med["atrous_dual_unguided"]
        # the check costs less than the two passes between checks while p > check / (2 * a pass over the whole frame)
        result["break_even_live_fraction_spheres"] = {"%s_spi_%d" % (g, n): med["atrous_dual_" + g] / (2.0 * med["pass_%d_samples" % n])
                                                      for g in ("unguided", "guided") for n in (8, 64)}
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
