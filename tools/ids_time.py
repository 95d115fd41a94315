#!/usr/bin/env python3
"""What the first-hit ID pass and the matte cost at 1920x1080 (one GPU, one call), and how often four slots suffice:

    python tools/ids_time.py [--runs 9] [--slots-spp 500] [--out profiles/r29_ids/ids_time.json]

1. ReflectiveSpheres and the benchmark mesh scene (GoldDragon stand-in), 16 spp, 32 x 32 tiles: rmd_render_ids against rmd_render_features (with
   squares) of the same tiles and samples, alternated, `runs` times each after a warm-up of each (tools/features_time.py's method).
2. rmd_ids_matte of three objects and the miss over the spheres frame's words, beside a device-to-device copy of the ID buffer (40 bytes a pixel read
   and written; the matte reads 40 and writes 8), alternated likewise.
3. Both scenes at --slots-spp samples: the share of pixels with 1, 2, 3 and 4 used slots and with other != 0.
Every call is bracketed by HIP events recorded on the context's own stream (rmd_context_create_on_stream); medians and spreads are reported.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import abi, render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

from denoise_time import hip  # noqa: E402  (tools/ is this script's directory)
from features_time import stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--slots-spp", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H, spp = 1920, 1080, 16
    H_ = hip()
    H_.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
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
    result = {"width": W, "height": H, "spp": spp, "runs": a.runs, "id_pass": {}, "matte": {}, "slots": {}}
    fts = [render.FeatureBuffer(ctx, W, H) for _ in range(2)]
    ids = [render.IdBuffer(ctx, W, H) for _ in range(2)]
    try:
        for name, scene in (("gold_dragon_standin", scenes.gold_dragon_standin()), ("reflective_spheres", scenes.reflective_spheres())):
            ds = render.DeviceScene(ctx, scene)
            try:
                def features():
                    render.render_features(ctx, ds, cam, st, tiles, fts[0], 0, spp, features_sq=fts[1])

                def id_pass():
                    render.render_ids(ctx, ds, cam, st, tiles, ids[0], 0, spp)

                rec = {k: stats(v) for k, v in alternate({"feature_pass": features, "id_pass": id_pass}).items()}
                rec["id_over_feature_median"] = rec["id_pass"]["median_ms"] / rec["feature_pass"]["median_ms"]
                result["id_pass"][name] = rec
                print(name, json.dumps(rec), flush=True)
                # how often four slots suffice
                ids[1].zero()
                t0 = time.time()
                render.render_ids(ctx, ds, cam, st, tiles, ids[1], 0, a.slots_spp)
                words = ids[1].download()
                used = (words[..., 0:8:2] != 0).sum(axis=-1)
                n = float(W * H)
                slots = {"spp": a.slots_spp, "objects": len(scene.objects), "seconds": time.time() - t0,
                         "share_with_used_slots": {str(k): float((used == k).sum()) / n for k in (1, 2, 3, 4)},
                         "share_with_other": float((words[..., 8] != 0).sum()) / n, "pixels_with_other": int((words[..., 8] != 0).sum()),
                         "largest_other_share_of_a_pixel": float((words[..., 8] / np.maximum(words[..., 9], 1)).max()),
                         "share_of_samples_that_miss": float(np.where(words[..., 0:8:2] == abi.RMD_ID_MISS, words[..., 1:8:2], 0).sum()) / (n * a.slots_spp)}
                assert (words[..., 9] == a.slots_spp).all()
                result["slots"][name] = slots
                print(name, "slots", json.dumps(slots), flush=True)
                ids[0].zero()
                id_pass()  # (the timed calls went on counting: the last scene's 16 spp are what the matte gets)
            finally:
                ds.close()
        objects = np.array([0, 3, 5, abi.RMD_ID_MISS], dtype=np.uint32)
        matte = render.ErrorImage(ctx, W, H)
        other = C.c_uint64()
        n_bytes = W * H * abi.RMD_ID_WORDS * 4

        def matte_call():
            ctx.check(ctx.L.rmd_ids_matte(ctx.handle, ids[0].ptr, W, H, objects.ctypes.data_as(C.POINTER(C.c_uint32)), len(objects), matte.ptr, C.byref(other)))

        def copy():
            assert H_.hipMemcpyAsync(ids[1].ptr, ids[0].ptr, n_bytes, 3, stream) == 0  # hipMemcpyDeviceToDevice

        try:
            rec = {k: stats(v) for k, v in alternate({"rmd_ids_matte": matte_call, "copy_of_the_id_buffer": copy}).items()}
        finally:
            matte.close()
        rec["matte_bytes_moved"], rec["copy_bytes_moved"] = W * H * 48, 2 * n_bytes
        rec["matte_gb_per_s"] = rec["matte_bytes_moved"] / rec["rmd_ids_matte"]["median_ms"] / 1e6
        rec["copy_gb_per_s"] = rec["copy_bytes_moved"] / rec["copy_of_the_id_buffer"]["median_ms"] / 1e6
        rec["other_pixels"] = other.value
        result["matte"] = rec
        print("matte", json.dumps(rec), flush=True)
    finally:
        for b in fts + ids:
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
