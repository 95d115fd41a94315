#!/usr/bin/env python3
"""What rmd_denoise costs at 1920x1080 (one GPU):

    python tools/denoise_time.py [--runs 9] [--out profiles/r08_denoise/denoise_time.json]

The frame is ReflectiveSpheres 1920x1080 at 16 spp with moments (one rect).  The default parameters (r 10, f 3) and the limits (r 12, f 4) are
run alternately, `runs` times each after one warm-up call each; every call is bracketed by HIP events recorded on the context's own stream
(rmd_context_create_on_stream), so a time covers the call's stream work: the count-image memset and kernel and the filter kernel.  Wall
times of the synchronous call are reported beside them.  The kernel alone is timed by a separate run under rocprofv3 --kernel-trace --stats
(--rocprof-child runs the calls without the event bracketing, for that).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

PARAMS = {"default": dict(radius=10, patch_radius=3, k=0.45, alpha=1.0), "limits": dict(radius=12, patch_radius=4, k=0.45, alpha=1.0)}


def hip():
    L = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    for name in ("hipStreamCreate", "hipStreamDestroy", "hipEventCreate", "hipEventRecord", "hipEventSynchronize", "hipEventElapsedTime",
                 "hipEventDestroy"):
        getattr(L, name).restype = C.c_int
    return L


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
    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=scenes.SEED)
    ds = render.DeviceScene(ctx, scenes.reflective_spheres())
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(3)]
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert H_.hipEventCreate(C.byref(e)) == 0
    result = {"width": W, "height": H, "spp": spp, "scene": "reflective_spheres", "runs": a.runs, "params": PARAMS}
    try:
        render.render_tiles(ctx, ds, st.camera_settings, st, generate_tiles(W, H, (32, 32)), fbs[0], 0, spp, framebuffer_sq=fbs[1])
        rect, count = [(0, 0, W, H)], [spp]
        for name in PARAMS:  # warm-up: first launches set up the kernel's LDS attribute and the code object
            render.denoise(ctx, fbs[0], fbs[1], rect, count, fbs[2], **PARAMS[name])
        if a.rocprof_child:
            for r in range(a.runs):
                for name in PARAMS:
                    render.denoise(ctx, fbs[0], fbs[1], rect, count, fbs[2], **PARAMS[name])
            print("rocprof child done")
            return
        ms = {n: [] for n in PARAMS}
        wall = {n: [] for n in PARAMS}
        frames = {}
        for r in range(a.runs):
            for name in (list(PARAMS) if r % 2 == 0 else list(reversed(PARAMS))):  # alternated: drift falls on both alike
                t0 = time.perf_counter()
                H_.hipEventRecord(ev[0], stream)
                render.denoise(ctx, fbs[0], fbs[1], rect, count, fbs[2], **PARAMS[name])
                H_.hipEventRecord(ev[1], stream)
                H_.hipEventSynchronize(ev[1])
                wall[name].append((time.perf_counter() - t0) * 1e3)
                f = C.c_float()
                H_.hipEventElapsedTime(C.byref(f), ev[0], ev[1])
                ms[name].append(f.value)
                if r == 0:
                    frames[name] = fbs[2].download()
        for name in PARAMS:
            v = ms[name]
            result[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_pct": 100.0 * (max(v) - min(v)) / min(v),
                            "runs_ms": v, "wall_median_ms": statistics.median(wall[name]), "wall_runs_ms": wall[name],
                            "finite_fraction": float((frames[name] == frames[name]).mean())}
    finally:
        for fb in fbs:
            fb.close()
        ds.close()
        ctx.close()
        for e in ev:
            H_.hipEventDestroy(e)
        H_.hipStreamDestroy(stream)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
