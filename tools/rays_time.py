#!/usr/bin/env python3
"""What closest-hit queries for caller-supplied rays cost at 1920x1080 rays (one GPU, one call):

    python tools/rays_time.py [--runs 9] [--warmup 40] [--out profiles/r32_rays/rays_time.json]

On ReflectiveSpheres and the benchmark mesh scene (GoldDragon stand-in): rmd_intersect_rays on the frame's pixel-centre primary rays (made on the device by
rmd_camera_rays) in three orders — row-major, 8 x 8 tile order (a wave's 64 rays are one wave tile's, as in the first-hit passes) and a seeded random
order — against rmd_render_ids at 1 spp over the same frame in 32 x 32 tiles, which performs the same intersections: the four alternated, `runs` times
each after `warmup` calls of each (tools/ao_time.py's method).  And rmd_camera_rays alone, which uploads its 8 bytes of pixel a
ray from pageable host memory inside the call.
Every call is bracketed by HIP events recorded on the context's own stream (rmd_context_create_on_stream); medians and spreads are reported.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

from denoise_time import hip  # noqa: E402  (tools/ is this script's directory)
from features_time import stats  # noqa: E402


def orders(W, H):
    """pixel (x, y) lists of the frame: row-major, 8 x 8 tile order (tiles row-major, pixels row-major inside a tile), and a seeded shuffle"""
    ys, xs = np.mgrid[0:H, 0:W]
    rows = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.uint32)
    assert W % 8 == 0 and H % 8 == 0
    t = rows.reshape(H // 8, 8, W // 8, 8, 2).transpose(0, 2, 1, 3, 4).reshape(-1, 2)
    return {"row_major": rows, "tile_order": np.ascontiguousarray(t), "random_order": rows[np.random.default_rng(0x1257).permutation(len(rows))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=40, help="calls of every series before the timed ones")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = 1920, 1080
    n = W * H
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
        for _ in range(a.warmup):  # warm-up: code objects, LDS attributes — and the clocks: a pass of under a millisecond does not bring them up in one call
            for fn in fns.values():
                fn()
        ctx.synchronize()
        ms = {name: [] for name in fns}
        for r in range(a.runs):
            for name in (list(fns) if r % 2 == 0 else list(reversed(fns))):  # alternated: drift falls on all alike
                ms[name].append(timed(fns[name]))
        return ms

    st = Settings(scenes.camera(W, H), sample_count=1, bounce_limit=1, seed=scenes.SEED)
    cam = st.camera_settings
    tiles = generate_tiles(W, H, (32, 32))
    pixels = orders(W, H)
    result = {"width": W, "height": H, "rays": n, "runs": a.runs, "warmup_calls": a.warmup, "bytes_per_ray": 88, "intersect": {}, "camera_rays": {}}
    ids = render.IdBuffer(ctx, W, H)
    hits = render.HitBuffer(ctx, n)
    rays = {name: render.camera_rays(ctx, cam, xy) for name, xy in pixels.items()}
    try:
        for name, scene in (("gold_dragon_standin", scenes.gold_dragon_standin()), ("reflective_spheres", scenes.reflective_spheres())):
            ds = render.DeviceScene(ctx, scene)
            try:
                fns = {"id_pass_1spp": lambda: render.render_ids(ctx, ds, cam, st, tiles, ids, 0, 1)}
                for order in pixels:
                    fns[order] = lambda order=order: render.intersect_rays_dev(ctx, ds, rays[order], hits)
                rec = {k: stats(v) for k, v in alternate(fns).items()}
                for order in pixels:
                    rec[order + "_over_id_median"] = rec[order]["median_ms"] / rec["id_pass_1spp"]["median_ms"]
                    rec[order + "_mrays_per_s"] = n / rec[order]["median_ms"] / 1e3
                got = hits.download()  # (the last series run: the random order)
                rec["hit_share"] = float((got["object"] >= 0).mean())
                rec["on_a_triangle"] = float((got["triangle"] > 0).mean())
                result["intersect"][name] = rec
                print(name, json.dumps(rec), flush=True)
            finally:
                ds.close()
        xy = pixels["row_major"]
        rec = {k: stats(v) for k, v in alternate({"rmd_camera_rays": lambda: render.camera_rays(ctx, cam, xy, out=rays["row_major"])}).items()}
        rec["bytes_uploaded"], rec["bytes_written"] = n * 8, n * 48
        result["camera_rays"] = rec
        print("camera_rays", json.dumps(rec), flush=True)
    finally:
        for b in [ids, hits] + list(rays.values()):
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
