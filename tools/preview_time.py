#!/usr/bin/env python3
"""What a frame preview costs, at 1920x1080 on one GPU:

    python tools/preview_time.py call [--runs 15] [--out profiles/r19_preview/call_time.json]
    python tools/preview_time.py loop [--runs 5] [--baseline-cli PATH] [--out profiles/r19_preview/loop_time.json]

call    ReflectiveSpheres at 16 spp in a device framebuffer; wall time around whole calls (each is synchronous and ends with its bytes on the host):
        rmd_resolve_tonemap — entered twice, as two series, so that their difference shows what two series of one call differ by —, and
        rmd_resolve_tonemap_tiles over the frame as one rect, over the 2,040 tiles of 32 x 32, and over a random quarter of them (numpy's
        default_rng(0)).  All five alternated, `runs` times each after a warm-up of each; medians with their spread.

loop    ReflectiveSpheres, 500 spp, 5 bounces, through the C++ host mirror's render_tiled as `raymond_cli hostapi` times it (a child process per
        run: from the call to the last TileFinished message, the best of its three renders): one pass; samples_per_iteration 8 with the defaults;
        with --progress-tiles 0; and with --progress-tiles 0 and a preview after every 1, 4 and 8 passes, raw and through the fast filter.  With
        --baseline-cli (a raymond_cli built from another commit) that binary's default progressive render is a series of its own.  All alternated,
        `runs` child processes each; medians with their spread, and every progressive figure's share of the one-pass rate.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "runs": len(s)}


def alternated(fns, runs, timed):
    ms = {n: [] for n in fns}
    for r in range(runs):
        for name in (list(fns) if r % 2 == 0 else list(reversed(fns))):  # alternated: drift falls on all alike
            ms[name].append(timed(fns[name]))
    out = {k: stats(v) for k, v in ms.items()}
    for k, v in out.items():
        print(k, "%.3f ms (min %.3f, max %.3f)" % (v["median_ms"], v["min_ms"], v["max_ms"]), flush=True)
    return out


def call_times(a):
    import ctypes as C

    import numpy as np

    from raymond_amd import render, scenes
    from raymond_amd.scene import Settings, generate_tiles, tile_array

    spp = 16
    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=scenes.SEED)
    tiles = generate_tiles(W, H, (32, 32))
    rng = np.random.default_rng(0)
    quarter = [tiles[i] for i in sorted(rng.choice(len(tiles), size=len(tiles) // 4, replace=False))]
    result = {"width": W, "height": H, "spp": spp, "tiles": len(tiles), "quarter_tiles": len(quarter),
              "quarter_pixel_fraction": sum(w * h for (_, _, w, h) in quarter) / float(W * H)}
    with render.Context(0) as ctx:
        ds, fb = render.DeviceScene(ctx, scenes.reflective_spheres()), render.Framebuffer(ctx, W, H)
        try:
            render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fb)
            # the C calls themselves, their arguments made beforehand (the Python mirror's per-rect work is not what is timed)
            def c_call(rects):
                n = sum(w * h for (_, _, w, h) in rects)
                arr, counts, out = tile_array(rects), np.full(len(rects), spp, dtype=np.uint32), np.empty(n * 3, dtype=np.uint8)
                args = (ctx.handle, fb.ptr, None, W, H, arr, counts.ctypes.data_as(C.POINTER(C.c_uint32)), len(rects), 1.0, 2.2, out.ctypes.data_as(C.c_void_p))
                return lambda: ctx.check(ctx.L.rmd_resolve_tonemap_tiles(*args)) or (out, counts)

            whole_out = np.empty(W * H * 3, dtype=np.uint8)

            def whole_call():
                ctx.check(ctx.L.rmd_resolve_tonemap(ctx.handle, fb.ptr, W, H, spp, 1.0, 2.2, whole_out.ctypes.data_as(C.c_void_p)))

            fns = {"resolve_tonemap_series_a": whole_call, "tiles_one_rect": c_call([(0, 0, W, H)]), "tiles_2040_tiles": c_call(tiles),
                   "tiles_random_quarter": c_call(quarter), "resolve_tonemap_series_b": whole_call}
            for fn in fns.values():
                fn()  # warm-up: code objects, the context's scratch
            whole = render.resolve_tonemap(ctx, fb, spp)
            assert np.array_equal(fns["tiles_one_rect"]()[0].reshape(H, W, 3), whole)
            assert np.array_equal(render.scatter_tiles(tiles, render.resolve_tonemap_tiles(ctx, fb, tiles, [spp] * len(tiles)), W, H), whole)

            def timed(fn):
                t0 = time.perf_counter()
                fn()
                return (time.perf_counter() - t0) * 1e3

            result["calls"] = alternated(fns, a.runs, timed)
        finally:
            fb.close(), ds.close()
    med = {k: v["median_ms"] for k, v in result["calls"].items()}
    result["series_b_over_series_a"] = med["resolve_tonemap_series_b"] / med["resolve_tonemap_series_a"]
    result["one_rect_over_resolve_tonemap"] = med["tiles_one_rect"] / med["resolve_tonemap_series_a"]
    result["quarter_over_all_tiles"] = med["tiles_random_quarter"] / med["tiles_2040_tiles"]
    return result


def loop_times(a):
    cli = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
    base = ["hostapi", "spheres", str(W), str(H), "500", "5"]
    runs = {"one_pass": [cli] + base + ["0"], "progressive_defaults": [cli] + base + ["8"],
            "no_progress_tiles": [cli] + base + ["8", "--progress-tiles", "0"]}
    if a.baseline_cli:
        runs["baseline_progressive_defaults"] = [a.baseline_cli] + base + ["8"]
    for every in (1, 4, 8):
        for name, extra in (("raw", []), ("denoised", ["--preview-denoise", "1"])):
            runs["preview_every_%d_%s" % (every, name)] = [cli] + base + ["8", "--progress-tiles", "0", "--preview-every", str(every)] + extra
    lines = {}

    def timed(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError("%s: %s" % (" ".join(cmd), r.stderr[-2000:]))
        line = json.loads(r.stdout.strip().split("\n")[-1])
        lines[" ".join(cmd[1:])] = line
        return line["wall_ms"]

    result = {"width": W, "height": H, "spp": 500, "bounces": 5, "samples_per_iteration": 8, "how": "raymond_cli hostapi: wall_ms, the best of its three renders, per child process",
              "renders": alternated(runs, a.runs, timed)}
    med = {k: v["median_ms"] for k, v in result["renders"].items()}
    result["share_of_one_pass_rate"] = {k: med["one_pass"] / v for k, v in med.items() if k != "one_pass"}
    result["messages"] = {k: {"tile_progressed_messages": v["tile_progressed_messages"], "frame_previews": v.get("frame_previews", 0)} for k, v in lines.items()}
    print(json.dumps(result["share_of_one_pass_rate"]), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["call", "loop"])
    ap.add_argument("--runs", type=int, default=None)
    ap.add_argument("--baseline-cli", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs is None:
        a.runs = 15 if a.what == "call" else 5
    result = call_times(a) if a.what == "call" else loop_times(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
