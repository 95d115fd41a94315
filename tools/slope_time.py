#!/usr/bin/env python3
"""What the feature-slope term costs at 1920x1080 (one GPU, one call):

    python tools/slope_time.py [--runs 7] [--out profiles/r20_slope/slope_time.json]
    RAYMOND_HIP_LIB=<a build of the parent commit> python tools/slope_time.py --existing-only [--out profiles/r20_slope/slope_time_parent.json]

ReflectiveSpheres, 16 spp in two halves of 8 (samples 0..7 and 8..15) with the first-hit features of all 16, one full-frame rect, r = 10, f = 3, the
shipped k, k_f and tau.  For each of the four filters — rmd_denoise_guided, rmd_denoise_dual_guided, its region form over every other 32 x 32 tile,
rmd_denoise_dual_select at the default candidates and both windows 2 — three calls are alternated, `runs` times each after a warm-up of each: the
existing entry point, the _slope entry point at slope 0 and the _slope entry point at slope 3.  Every call is the WHOLE call (scratch, planes, kernels,
the wait), bracketed by HIP events recorded on the context's own stream; medians with min and max are reported.
--existing-only times the existing entry points alone: with RAYMOND_HIP_LIB set to a build of the parent commit, what they cost before this change.
--filter NAME times that filter alone: what a `rocprofv3 --kernel-trace --stats` run wraps to tell the kernels' time from the rest of the call.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import lib, render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

from denoise_time import hip  # noqa: E402  (tools/ is this script's directory)


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_pct": 100.0 * (max(v) - min(v)) / min(v), "runs_ms": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--existing-only", action="store_true")
    ap.add_argument("--filter", default=None, help="time this filter alone (e.g. rmd_denoise_guided)")
    a = ap.parse_args()
    if a.existing_only:  # a parent build has no _slope symbols: declare only what it exports
        for name in [n for n in lib.SIGNATURES if "_slope" in n]:
            del lib.SIGNATURES[name]
    W, H, spp, half = 1920, 1080, 16, 8
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
        return ms

    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=scenes.SEED)
    cam = st.camera_settings
    tiles = generate_tiles(W, H, (32, 32))
    result = {"width": W, "height": H, "spp": spp, "runs": a.runs, "library": "the build named by RAYMOND_HIP_LIB" if os.environ.get("RAYMOND_HIP_LIB") else "the in-tree build", "filters": {}}
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(7)]  # S_A, Q_A, S_B, Q_B, S, Q, out
    fts = [render.FeatureBuffer(ctx, W, H) for _ in range(2)]
    err = render.ErrorImage(ctx, W, H)
    try:
        ds = render.DeviceScene(ctx, scenes.reflective_spheres())
        try:
            render.render_tiles(ctx, ds, cam, st, tiles, fbs[0], 0, half, framebuffer_sq=fbs[1])
            render.render_tiles(ctx, ds, cam, st, tiles, fbs[2], half, half, framebuffer_sq=fbs[3])
            render.render_tiles(ctx, ds, cam, st, tiles, fbs[4], 0, spp, framebuffer_sq=fbs[5])
            render.render_features(ctx, ds, cam, st, tiles, fts[0], 0, spp, features_sq=fts[1])
        finally:
            ds.close()
        rect = [(0, 0, W, H)]
        guide = dict(k_f=st.denoise_feature_k, tau=st.denoise_feature_tau)
        dual = dict(features=fts[0], features_sq=fts[1], counts_f=[spp], **guide)
        A, B = (fbs[0], fbs[1]), (fbs[2], fbs[3])
        region = tiles[::2]

        def single(**kw):
            return lambda: render.denoise_guided(ctx, fbs[4], fbs[5], fts[0], fts[1], rect, [spp], fbs[6], **guide, **kw)

        def dual_call(reg, **kw):
            return lambda: render.denoise_dual(ctx, A, B, rect, [half], [half], fbs[6], err, region=reg, **dual, **kw)

        def select(slope):
            cands = [dict(c) for c in st.select_candidates()]
            if slope is not None:
                cands[1]["slope"] = slope
            return lambda: render.denoise_dual_select(ctx, A, B, rect, [half], [half], cands, fbs[6], err, features=fts[0], features_sq=fts[1], counts_f=[spp])

        filters = {"rmd_denoise_guided": lambda s: single(**({} if s is None else dict(slope=s))),
                   "rmd_denoise_dual_guided": lambda s: dual_call(None, **({} if s is None else dict(slope=s))),
                   "rmd_denoise_dual_guided_region": lambda s: dual_call(region, **({} if s is None else dict(slope=s))),
                   "rmd_denoise_dual_select": select}
        for name, make in filters.items():
            if a.filter and name != a.filter:
                continue
            fns = {"existing": make(None)}
            if not a.existing_only:
                fns.update(slope_0=make(0.0), slope_3=make(3.0))
            rec = {k: stats(v) for k, v in alternate(fns).items()}
            if not a.existing_only:
                rec["slope_3_over_slope_0_median"] = rec["slope_3"]["median_ms"] / rec["slope_0"]["median_ms"]
                rec["slope_0_over_existing_median"] = rec["slope_0"]["median_ms"] / rec["existing"]["median_ms"]
                rec["slope_3_minus_slope_0_ms"] = rec["slope_3"]["median_ms"] - rec["slope_0"]["median_ms"]
            result["filters"][name] = rec
            print(name, json.dumps({k: (v if not isinstance(v, dict) else {q: v[q] for q in ("median_ms", "min_ms", "max_ms")}) for k, v in rec.items()}), flush=True)
    finally:
        for b in fbs + fts + [err]:
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
