#!/usr/bin/env python3
"""What the ambient-occlusion pass and its resolve cost at 1920x1080 (one GPU, one call):

    python tools/ao_time.py [--runs 9] [--warmup 40] [--out profiles/r31_ao/ao_time.json]

1. ReflectiveSpheres and the benchmark mesh scene (GoldDragon stand-in), 16 spp, 32 x 32 tiles: rmd_render_ao at max_distance 1.0 and at +inf against
   rmd_render_ids of the same tiles and samples, the three alternated, `runs` times each after `warmup` calls of each (tools/ids_time.py's method with a longer warm-up,
   DESIGN.md section 34); and the shares of the samples that are occluded, open and none at either distance.
2. rmd_ao_resolve over the last frame's words (16 bytes a pixel read, 8 written).
Every call is bracketed by HIP events recorded on the context's own stream (rmd_context_create_on_stream); medians and spreads are reported.
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
from features_time import stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=40, help="calls of every series before the timed ones")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H, spp = 1920, 1080, 16
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
        for _ in range(a.warmup):  # warm-up: code objects, LDS attributes, scratch — and the clocks: a pass of under a millisecond does not bring them up in one call
            for fn in fns.values():
                fn()
        ctx.synchronize()
        ms = {n: [] for n in fns}
        for r in range(a.runs):
            for name in (list(fns) if r % 2 == 0 else list(reversed(fns))):  # alternated: drift falls on all alike
                ms[name].append(timed(fns[name]))
        return ms

    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=scenes.SEED)
    cam = st.camera_settings
    tiles = generate_tiles(W, H, (32, 32))
    result = {"width": W, "height": H, "spp": spp, "runs": a.runs, "warmup_calls": a.warmup, "ao_pass": {}, "resolve": {}}
    ids = render.IdBuffer(ctx, W, H)
    ao = [render.AoBuffer(ctx, W, H) for _ in range(2)]
    try:
        for name, scene in (("gold_dragon_standin", scenes.gold_dragon_standin()), ("reflective_spheres", scenes.reflective_spheres())):
            ds = render.DeviceScene(ctx, scene)
            try:
                def id_pass():
                    render.render_ids(ctx, ds, cam, st, tiles, ids, 0, spp)

                def ao_1():
                    render.render_ao(ctx, ds, cam, st, tiles, 1.0, ao[0], 0, spp)

                def ao_inf():
                    render.render_ao(ctx, ds, cam, st, tiles, float("inf"), ao[1], 0, spp)

                rec = {k: stats(v) for k, v in alternate({"id_pass": id_pass, "ao_pass_distance_1": ao_1, "ao_pass_distance_inf": ao_inf}).items()}
                for k in ("ao_pass_distance_1", "ao_pass_distance_inf"):
                    rec[k + "_over_id_median"] = rec[k]["median_ms"] / rec["id_pass"]["median_ms"]
                for k, buf, fn in (("distance_1", ao[0], ao_1), ("distance_inf", ao[1], ao_inf)):
                    buf.zero()
                    fn()  # (the timed calls went on counting: one call's words)
                    words = buf.download()
                    n = float(W * H * spp)
                    assert (words[..., 3] == spp).all()
                    rec["shares_" + k] = {w: float(words[..., j].sum()) / n for j, w in enumerate(("occluded", "open", "none"))}
                result["ao_pass"][name] = rec
                print(name, json.dumps(rec), flush=True)
            finally:
                ds.close()
        out = render.ErrorImage(ctx, W, H)
        empty = C.c_uint64()

        def resolve():
            ctx.check(ctx.L.rmd_ao_resolve(ctx.handle, ao[0].ptr, W, H, 1.0, out.ptr, C.byref(empty)))

        try:
            rec = {k: stats(v) for k, v in alternate({"rmd_ao_resolve": resolve}).items()}
        finally:
            out.close()
        rec["bytes_moved"] = W * H * 24
        rec["gb_per_s"] = rec["bytes_moved"] / rec["rmd_ao_resolve"]["median_ms"] / 1e6
        rec["empty_pixels"] = empty.value
        result["resolve"] = rec
        print("resolve", json.dumps(rec), flush=True)
    finally:
        for b in [ids] + ao:
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
