#!/usr/bin/env python3
"""What rmd_luminance_histogram_tiles costs, and what exposure it asks for, at 1920x1080 on one GPU:

    python tools/luma_histogram_time.py call [--runs 15] [--out profiles/r22_luma_histogram/call_time.json]
    python tools/luma_histogram_time.py exposures [--out profiles/r22_luma_histogram/exposures.json]

call        Three frames of sums in a device framebuffer — ReflectiveSpheres rendered at 16 spp, a frame of one constant value (every pixel in one bin:
            the worst contention), a frame of uniformly random exponents (2^-40 .. 2^40: the most distinct bins a wave can hold) — and three rect lists:
            the frame as one rect, its 2,040 tiles of 32 x 32, a random quarter of them (numpy's default_rng(0)).  For each of the nine pairs
            rmd_luminance_histogram_tiles and rmd_resolve_tonemap_tiles, which reads the same bytes, are timed around the whole call (each is
            synchronous): HIP events recorded on the context's stream in front of and behind the call, and the wall clock.  All eighteen alternated,
            `runs` times each after a warm-up of each; medians with their spread.  Every histogram is first held against the numpy restatement
            (tests/luma_ref.py) at this size.
exposures   rmd_exposure_from_histogram at the starting values (percentile 0.99, target 0.8) for the two bundled scenes at 16 and 500 spp, 5 bounces.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
W, H = 1920, 1080


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "runs": len(s)}


class Hip:
    """The few runtime calls the event timing needs, from the runtime the library has loaded."""

    def __init__(self):
        self.rt = C.CDLL("libamdhip64.so")

    def ok(self, status, what):
        if status != 0:
            raise RuntimeError("%s failed with HIP error %d" % (what, status))

    def stream(self):
        s = C.c_void_p()
        self.ok(self.rt.hipStreamCreate(C.byref(s)), "hipStreamCreate")
        return s

    def event(self):
        e = C.c_void_p()
        self.ok(self.rt.hipEventCreate(C.byref(e)), "hipEventCreate")
        return e

    def timed(self, stream, start, stop, fn):
        """(HIP-event ms, wall ms) around fn()"""
        self.ok(self.rt.hipEventRecord(start, stream), "hipEventRecord")
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        self.ok(self.rt.hipEventRecord(stop, stream), "hipEventRecord")
        self.ok(self.rt.hipEventSynchronize(stop), "hipEventSynchronize")
        ms = C.c_float()
        self.ok(self.rt.hipEventElapsedTime(C.byref(ms), start, stop), "hipEventElapsedTime")
        return ms.value, wall


def call_times(a):
    import numpy as np

    import luma_ref
    from raymond_amd import abi, lib, render, scenes
    from raymond_amd.scene import Settings, generate_tiles, tile_array

    lib.load()
    hip = Hip()
    spp = 16
    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=scenes.SEED)
    tiles = generate_tiles(W, H, (32, 32))
    rng = np.random.default_rng(0)
    quarter = [tiles[i] for i in sorted(rng.choice(len(tiles), size=len(tiles) // 4, replace=False))]
    lists = {"one_rect": [(0, 0, W, H)], "2040_tiles": tiles, "random_quarter": quarter}
    result = {"width": W, "height": H, "spp": spp, "tiles": len(tiles), "quarter_tiles": len(quarter), "library": os.path.relpath(lib.LIB_PATH, ROOT),
              "how": "HIP events on the context's stream around the whole synchronous call (event_*), and the wall clock (wall_*); alternated, medians"}
    stream = hip.stream()
    with render.Context(0, stream=stream.value) as ctx:
        ds = render.DeviceScene(ctx, scenes.reflective_spheres())
        fbs = {name: render.Framebuffer(ctx, W, H) for name in ("rendered", "constant", "random_exponents")}
        try:
            render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fbs["rendered"])
            fbs["constant"].upload(np.full((H, W, 3), 0.05 * spp))
            fbs["random_exponents"].upload(np.exp2(rng.uniform(-40, 40, (H, W, 3))) * spp)
            fns, result["distinct_counters"] = {}, {}
            for fname, fb in fbs.items():
                acc = fb.download()
                for lname, rects in lists.items():
                    counts = np.full(len(rects), spp, dtype=np.uint32)
                    got, want = render.luminance_histogram(ctx, fb, rects, counts), luma_ref.histogram(acc, rects, counts)
                    assert got == want, (fname, lname)  # exact at the size that is timed
                    arr, cptr = tile_array(rects), counts.ctypes.data_as(C.POINTER(C.c_uint32))
                    out_h = abi.LumaHistogram()
                    out_b = np.empty(sum(w * h for (_, _, w, h) in rects) * 3, dtype=np.uint8)

                    def hist(fb=fb, arr=arr, cptr=cptr, n=len(rects), out_h=out_h, keep=counts):
                        ctx.check(ctx.L.rmd_luminance_histogram_tiles(ctx.handle, fb.ptr, None, W, H, arr, cptr, n, C.byref(out_h)))

                    def resolve(fb=fb, arr=arr, cptr=cptr, n=len(rects), out_b=out_b, keep=counts):
                        ctx.check(ctx.L.rmd_resolve_tonemap_tiles(ctx.handle, fb.ptr, None, W, H, arr, cptr, n, 1.0, 2.2, out_b.ctypes.data_as(C.c_void_p)))

                    fns["histogram %s %s" % (fname, lname)] = hist
                    fns["resolve %s %s" % (fname, lname)] = resolve
                result["distinct_counters"][fname] = int(np.count_nonzero(want.counters()[:261]))
            for fn in fns.values():
                fn()  # warm-up: code objects, the context's scratch
            start, stop = hip.event(), hip.event()
            ev, wall = {n: [] for n in fns}, {n: [] for n in fns}
            for r in range(a.runs):
                for name in (list(fns) if r % 2 == 0 else list(reversed(fns))):  # alternated: drift falls on all alike
                    e, w = hip.timed(stream, start, stop, fns[name])
                    ev[name].append(e), wall[name].append(w)
            result["calls"] = {n: {"event": stats(ev[n]), "wall": stats(wall[n])} for n in fns}
            for n, v in result["calls"].items():
                print("%-44s event %.3f ms (min %.3f, max %.3f)  wall %.3f ms" % (n, v["event"]["median_ms"], v["event"]["min_ms"], v["event"]["max_ms"],
                                                                                 v["wall"]["median_ms"]), flush=True)
            result["histogram_over_resolve"] = {n[len("histogram "):]: v["event"]["median_ms"] / result["calls"]["resolve " + n[len("histogram "):]]["event"]["median_ms"]
                                                for n, v in result["calls"].items() if n.startswith("histogram ")}
            print(json.dumps(result["histogram_over_resolve"]), flush=True)
        finally:
            for fb in fbs.values():
                fb.close()
            ds.close()
    return result


def exposures(a):
    import numpy as np

    from raymond_amd import render, scenes
    from raymond_amd.scene import Settings, generate_tiles

    tiles = generate_tiles(W, H, (32, 32))
    result = {"width": W, "height": H, "bounces": 5, "percentile": 0.99, "target": 0.8, "scenes": {}}
    with render.Context(0) as ctx:
        for name, scene in (("reflective_spheres", scenes.reflective_spheres()), ("gold_dragon_standin", scenes.gold_dragon_standin())):
            ds, fb = render.DeviceScene(ctx, scene), render.Framebuffer(ctx, W, H)
            try:
                done = 0
                for spp in (16, 500):
                    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=scenes.SEED)
                    render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fb, done, spp - done)  # (the samples [done, spp) on top of the first 16)
                    done = spp
                    h = render.luminance_histogram(ctx, fb, [(0, 0, W, H)], [spp])
                    e = render.exposure_from_histogram(h)
                    top = int(np.flatnonzero(h.bins)[-1]) if h.bins.any() else None
                    result["scenes"]["%s %d spp" % (name, spp)] = {"exposure": e, "brightest_bin": top, "below": h.below, "above": h.above, "zero": h.zero,
                                                                   "negative": h.negative, "not_finite": h.not_finite,
                                                                   "bins": {int(i): int(h.bins[i]) for i in np.flatnonzero(h.bins)}}
                    print(name, spp, "spp: exposure %.6f, brightest bin %s, zero %d" % (e, top, h.zero), flush=True)
            finally:
                fb.close(), ds.close()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["call", "exposures"])
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = call_times(a) if a.what == "call" else exposures(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
