#!/usr/bin/env python3
"""What rmd_despike costs at 1920x1080 on one GPU:

    python tools/despike_time.py [--runs 15] [--out profiles/r23_despike/call_time.json]

ReflectiveSpheres rendered at 16 spp with its second moments, as one rect and as its 2,040 tiles of 32 x 32.  For each list three things are timed around
the whole call, with HIP events recorded on the context's stream in front of and behind it and with the wall clock: rmd_despike at the starting values
(radius 2, rank 2, k 6, ratio 2, floor 0) with its per-rect counts, rmd_resolve_tonemap_tiles on the same list, and — the floor — the device-to-device
copies of S to S' and Q to Q', the 199 MB the call has to read and write.  rmd_despike is also timed at radius 1 and 3 and without the counts.  All series
alternated, `runs` times each after a warm-up of each; medians with their spread.  Before anything is timed the call is held to the numpy restatement
(tests/despike_ref.py) on a 256 x 144 crop of the same frame, tiles and all."""
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
    """The few runtime calls the event timing and the copy need, from the runtime the library has loaded."""

    def __init__(self):
        self.rt = C.CDLL("libamdhip64.so")
        self.rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

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

    def copy(self, stream, dst, src, n_bytes):
        self.ok(self.rt.hipMemcpyAsync(dst, src, n_bytes, 3, stream), "hipMemcpyAsync")  # hipMemcpyDeviceToDevice

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np

    import despike_ref
    from raymond_amd import lib, render, scenes
    from raymond_amd.scene import Settings, generate_tiles, tile_array

    lib.load()
    hip = Hip()
    spp = 16
    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=scenes.SEED)
    tiles = generate_tiles(W, H, (32, 32))
    lists = {"one_rect": [(0, 0, W, H)], "2040_tiles": tiles}
    n_bytes = W * H * 3 * 8
    result = {"width": W, "height": H, "spp": spp, "tiles": len(tiles), "library": os.path.relpath(lib.LIB_PATH, ROOT), "bytes_read_and_written": 4 * n_bytes,
              "how": "HIP events on the context's stream around the whole synchronous call (event), and the wall clock (wall); alternated, medians"}
    stream = hip.stream()
    with render.Context(0, stream=stream.value) as ctx:
        ds = render.DeviceScene(ctx, scenes.reflective_spheres())
        fbs = [render.Framebuffer(ctx, W, H) for _ in range(4)]  # S, Q, S', Q'
        try:
            render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fbs[0], framebuffer_sq=fbs[1])
            # exact on a crop first: 256 x 144 from the frame's middle, as its own 32 x 32 tiles
            S, Q = fbs[0].download(), fbs[1].download()
            cs, cq = S[468:612, 832:1088].copy(), Q[468:612, 832:1088].copy()
            crop_tiles = generate_tiles(256, 144, (32, 32))
            got = render.despike_arrays(ctx, cs, cq, crop_tiles, [spp] * len(crop_tiles))
            want = despike_ref.despike(cs, cq, crop_tiles, [spp] * len(crop_tiles))
            assert despike_ref.same_bits(got[0], want[0]) and despike_ref.same_bits(got[1], want[1]) and list(got[2]) == list(want[2])
            result["crop_replaced"] = int(got[2].sum())
            fns = {}
            for lname, rects in lists.items():
                counts = np.full(len(rects), spp, dtype=np.uint32)
                arr, cptr = tile_array(rects), counts.ctypes.data_as(C.POINTER(C.c_uint32))
                replaced = np.zeros(len(rects), dtype=np.uint32)
                out_b = np.empty(sum(w * h for (_, _, w, h) in rects) * 3, dtype=np.uint8)

                def despike(radius=2, rank=2, with_counts=True, arr=arr, cptr=cptr, n=len(rects), replaced=replaced, keep=counts):
                    ctx.check(ctx.L.rmd_despike(ctx.handle, fbs[0].ptr, fbs[1].ptr, W, H, arr, cptr, n, radius, rank, 6.0, 2.0, 0.0, fbs[2].ptr, fbs[3].ptr,
                                                replaced.ctypes.data_as(C.POINTER(C.c_uint32)) if with_counts else None))

                def resolve(arr=arr, cptr=cptr, n=len(rects), out_b=out_b, keep=counts):
                    ctx.check(ctx.L.rmd_resolve_tonemap_tiles(ctx.handle, fbs[0].ptr, None, W, H, arr, cptr, n, 1.0, 2.2, out_b.ctypes.data_as(C.c_void_p)))

                fns["despike %s" % lname] = despike
                fns["despike radius 1 %s" % lname] = lambda f=despike: f(radius=1)
                fns["despike radius 3 %s" % lname] = lambda f=despike: f(radius=3)
                fns["despike without counts %s" % lname] = lambda f=despike: f(with_counts=False)
                fns["resolve %s" % lname] = resolve
                despike()
                result["replaced %s" % lname] = int(replaced.sum())

            def copy():
                hip.copy(stream, fbs[2].ptr, fbs[0].ptr, n_bytes), hip.copy(stream, fbs[3].ptr, fbs[1].ptr, n_bytes)
                ctx.synchronize()

            fns["device-to-device copy of S and Q"] = copy
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
            med = lambda n: result["calls"][n]["event"]["median_ms"]  # noqa: E731
            result["despike_over_resolve"] = {l: med("despike " + l) / med("resolve " + l) for l in lists}
            result["despike_over_copy"] = {l: med("despike " + l) / med("device-to-device copy of S and Q") for l in lists}
            print(json.dumps({"over_resolve": result["despike_over_resolve"], "over_copy": result["despike_over_copy"]}), flush=True)
        finally:
            for fb in fbs:
                fb.close()
            ds.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
