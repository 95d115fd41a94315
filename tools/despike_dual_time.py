#!/usr/bin/env python3
"""What rmd_despike_dual costs at 1920x1080 on one GPU:

    python tools/despike_dual_time.py [--runs 15] [--out profiles/r28_despike_dual/call_time.json]

ReflectiveSpheres rendered at 16 + 16 spp with its second moments into two halves, as one rect and as its 2,040 tiles of 32 x 32.  For each list, timed
around the whole call with HIP events recorded on the context's stream in front of and behind it and with the wall clock (tools/despike_time.py's method):
rmd_despike_dual at the starting values (radius 2, rank 2, k 6, ratio 2, floor 0) with its per-rect counts, at radius 1 and 3, and without the counts; and
what a caller has without the call: two rmd_despike calls, one per half, and — the floor — the device-to-device copies of the four buffers, the 398 MB the
call has to read and write.  All series alternated, `runs` times each after a warm-up of each; medians with their spread.  Before anything is timed the
call is held to the numpy restatement (tests/despike_dual_ref.py) on a 256 x 144 crop of the same frame, tiles and all."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np

    import despike_dual_ref
    from despike_time import Hip, stats
    from raymond_amd import lib, render, scenes
    from raymond_amd.scene import Settings, generate_tiles, tile_array

    lib.load()
    hip = Hip()
    spp = 16
    st = Settings(scenes.camera(W, H), sample_count=2 * spp, bounce_limit=5, seed=scenes.SEED)
    tiles = generate_tiles(W, H, (32, 32))
    lists = {"one_rect": [(0, 0, W, H)], "2040_tiles": tiles}
    n_bytes = W * H * 3 * 8
    result = {"width": W, "height": H, "spp_per_half": spp, "tiles": len(tiles), "library": os.path.relpath(lib.LIB_PATH, ROOT), "bytes_read_and_written": 8 * n_bytes,
              "how": "HIP events on the context's stream around the whole synchronous call (event), and the wall clock (wall); alternated, medians"}
    stream = hip.stream()
    with render.Context(0, stream=stream.value) as ctx:
        ds = render.DeviceScene(ctx, scenes.reflective_spheres())
        fbs = [render.Framebuffer(ctx, W, H) for _ in range(8)]  # S_A, Q_A, S_B, Q_B and the four outputs
        try:
            render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fbs[0], 0, spp, framebuffer_sq=fbs[1])
            render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fbs[2], spp, spp, framebuffer_sq=fbs[3])
            # exact on a crop first: 256 x 144 from the frame's middle, as its own 32 x 32 tiles
            crop = [fb.download()[468:612, 832:1088].copy() for fb in fbs[:4]]
            crop_tiles = generate_tiles(256, 144, (32, 32))
            counts = [spp] * len(crop_tiles)
            got = render.despike_dual_arrays(ctx, *crop, crop_tiles, counts, counts)
            want = despike_dual_ref.despike_dual(*crop, crop_tiles, counts, counts)
            assert all(despike_dual_ref.same_bits(g, w) for g, w in zip(got[:4], want[:4])) and list(got[4]) == list(want[4])
            result["crop_replaced"] = int(got[4].sum())
            fns = {}
            u32p = C.POINTER(C.c_uint32)
            for lname, rects in lists.items():
                counts = np.full(len(rects), spp, dtype=np.uint32)
                arr, cptr = tile_array(rects), counts.ctypes.data_as(u32p)
                replaced = np.zeros(len(rects), dtype=np.uint32)

                def dual(radius=2, rank=2, with_counts=True, arr=arr, cptr=cptr, n=len(rects), replaced=replaced, keep=counts):
                    ctx.check(ctx.L.rmd_despike_dual(ctx.handle, fbs[0].ptr, fbs[1].ptr, fbs[2].ptr, fbs[3].ptr, W, H, arr, cptr, cptr, n, radius, rank, 6.0, 2.0, 0.0, fbs[4].ptr,
                                                     fbs[5].ptr, fbs[6].ptr, fbs[7].ptr, replaced.ctypes.data_as(u32p) if with_counts else None))

                def single(half, with_counts=True, arr=arr, cptr=cptr, n=len(rects), replaced=replaced, keep=counts):
                    ctx.check(ctx.L.rmd_despike(ctx.handle, fbs[2 * half].ptr, fbs[2 * half + 1].ptr, W, H, arr, cptr, n, 2, 2, 6.0, 2.0, 0.0, fbs[4 + 2 * half].ptr,
                                                fbs[5 + 2 * half].ptr, replaced.ctypes.data_as(u32p) if with_counts else None))

                fns["despike_dual %s" % lname] = dual
                fns["despike_dual radius 1 %s" % lname] = lambda f=dual: f(radius=1)
                fns["despike_dual radius 3 %s" % lname] = lambda f=dual: f(radius=3)
                fns["despike_dual without counts %s" % lname] = lambda f=dual: f(with_counts=False)
                fns["one despike call %s" % lname] = lambda f=single: f(0)
                fns["two despike calls, one per half %s" % lname] = lambda f=single: (f(0), f(1))
                dual()
                result["replaced %s" % lname] = int(replaced.sum())

            def copy():
                for i in range(4):
                    hip.copy(stream, fbs[4 + i].ptr, fbs[i].ptr, n_bytes)
                ctx.synchronize()

            fns["device-to-device copy of the four buffers"] = copy
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
                print("%-52s event %.3f ms (min %.3f, max %.3f)  wall %.3f ms" % (n, v["event"]["median_ms"], v["event"]["min_ms"], v["event"]["max_ms"],
                                                                                 v["wall"]["median_ms"]), flush=True)
            med = lambda n: result["calls"][n]["event"]["median_ms"]  # noqa: E731
            result["dual_over_one_despike"] = {l: med("despike_dual " + l) / med("one despike call " + l) for l in lists}
            result["dual_over_two_despikes"] = {l: med("despike_dual " + l) / med("two despike calls, one per half " + l) for l in lists}
            result["dual_over_copy"] = {l: med("despike_dual " + l) / med("device-to-device copy of the four buffers") for l in lists}
            print(json.dumps({k: result[k] for k in ("dual_over_one_despike", "dual_over_two_despikes", "dual_over_copy")}), flush=True)
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
