#!/usr/bin/env python3
"""What the per-pixel choice among dual-buffer filters costs, at 1920x1080 (one GPU, one call):

    python tools/dual_select_time.py [--runs 9] [--out profiles/r13_select/dual_select_time.json]

ReflectiveSpheres, 16 + 16 samples in the two halves, the first-hit features of the same 32 samples, r = 10, f = 3, the 2,040 tiles of 32 x 32 as the
rects.  rmd_denoise_dual_select at the default candidates {k 0.45 unguided, k 1.0 guided, k_f 1.0, tau 1e-2}, both windows 2, with all of its outputs,
against rmd_denoise_dual and rmd_denoise_dual_guided on the same buffers (whose sum is what the two candidates cost as calls of their own), and
rmd_denoise_dual_select with either candidate alone — alternated, `runs` times each after a warm-up of each.  Every call is the WHOLE call, its
scratch allocation and copies included, bracketed by HIP events recorded on the context's own stream; medians and spreads are reported.
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
    err, sure, win = render.ErrorImage(ctx, W, H), render.ErrorImage(ctx, W, H), render.WinnerImage(ctx, W, H)
    cands = [dict(k=0.45, alpha=1.0), dict(k=1.0, alpha=1.0, guided=True, k_f=1.0, tau=1e-2)]
    result = {"width": W, "height": H, "runs": a.runs, "radius": 10, "patch_radius": 3, "candidates": cands, "sure_window": 2, "select_window": 2,
              "samples_per_half": 16, "feature_samples": 32, "tiles": len(tiles)}
    try:
        ds = render.DeviceScene(ctx, scenes.reflective_spheres())
        try:
            render.render_tiles(ctx, ds, cam, st, tiles, fbs[0], 0, 16, framebuffer_sq=fbs[1])
            render.render_tiles(ctx, ds, cam, st, tiles, fbs[2], 16, 16, framebuffer_sq=fbs[3])
            render.render_features(ctx, ds, cam, st, tiles, feat[0], 0, 32, features_sq=feat[1])
        finally:
            ds.close()
        guide = dict(features=feat[0], features_sq=feat[1], counts_f=n32)

        def select(cs):
            return lambda: render.denoise_dual_select(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), tiles, n16, n16, cs, fbs[4], err, sure, win, radius=10, patch_radius=3,
                                                      sure_window=2, select_window=2, **guide)

        def plain(guided):
            kw = dict(k=1.0, k_f=1.0, tau=1e-2, **guide) if guided else dict(k=0.45)
            return lambda: render.denoise_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), tiles, n16, n16, fbs[4], err, radius=10, patch_radius=3, alpha=1.0, **kw)

        fns = {"rmd_denoise_dual": plain(False), "rmd_denoise_dual_guided": plain(True), "rmd_denoise_dual_select": select(cands),
               "select_unguided_alone": select(cands[:1]), "select_guided_alone": select(cands[1:])}
        for fn in fns.values():
            fn()  # warm-up: code object, LDS attribute
        ms = {n: [] for n in fns}
        for r in range(a.runs):
            for name in (list(fns) if r % 2 == 0 else list(reversed(fns))):  # alternated: drift falls on all alike
                ms[name].append(timed(fns[name]))
        result["calls"] = {k: stats(v) for k, v in ms.items()}
        for k, v in result["calls"].items():
            print(k, "%.3f ms (min %.3f, max %.3f)" % (v["median_ms"], v["min_ms"], v["max_ms"]), flush=True)
        med = {k: v["median_ms"] for k, v in result["calls"].items()}
        both = med["rmd_denoise_dual"] + med["rmd_denoise_dual_guided"]
        result["sum_of_the_two_plain_calls_ms"] = both
        result["select_over_sum_of_the_two_plain_calls"] = med["rmd_denoise_dual_select"] / both
        result["select_minus_sum_of_the_two_plain_calls_ms"] = med["rmd_denoise_dual_select"] - both
    finally:
        for b in fbs + feat + [err, sure, win]:
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
