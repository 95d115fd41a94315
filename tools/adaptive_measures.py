#!/usr/bin/env python3
"""DESIGN.md section 10's table again, for the adaptive measures, and what rmd_tile_luma_error and rmd_tile_weighted_error cost:

    python tools/adaptive_measures.py table [--scene spheres|mesh] [--out profiles/r25_tile_weighted/table_spheres.json]
    python tools/adaptive_measures.py time  [--runs 15] [--out profiles/r25_tile_weighted/call_time.json]
    python tools/adaptive_measures.py dual-table [--out profiles/r27_tile_weighted_dual/table_dual.json]
    python tools/adaptive_measures.py dual-time  [--runs 15] [--out profiles/r27_tile_weighted_dual/call_time.json]

table: the scene at 1920x1080, up to 256 spp in passes of 16, 2,040 tiles of 32 x 32; RMSE against a 2,048 spp frame of another seed.  ONE progressive
render is made, every tile live to the end.  After every pass the three measures of every tile are taken (rmd_tile_error, and rmd_tile_luma_error's
tile_rms and pixel_rms) and the sums are kept.  A pixel's sums after k passes do not depend on which other tiles are live (raymond_hip.h:
rmd_render_tiles_moments), so the adaptive render at ANY threshold is read off these records exactly: a tile stops at the first check that finds its
measure at or below the threshold, and its pixels are the sums of that pass over that count.  Per measure the thresholds are the quantiles of the
measure's own values that bring the mean spp to about 245, 230, 215, 200, 180 and 160 — the three thresholds are not comparable numbers.  Each point:
tiles stopped early, mean spp, RMSE, and the RMSE of a uniform frame rendered at the same (rounded) mean spp.  One point per measure is then rendered
for real through render_tiled with Settings.adaptive_measure and must stop the same tiles at the same counts and give the frame's bytes.  A fourth
measure that is no setting is replayed beside them from the same records: sqrt(mean_variance), the tile's absolute RMS standard error of luminance.
A fifth, "display", is Settings.adaptive_display_threshold's: rmd_tile_weighted_error's rms under rmd_display_weights' table at exposure 1, gamma 2.2 and
floor 1 / 255 — the tile's RMS error after the tone curve; its loop check goes through that setting.  Every cell carries two errors: the RMSE in linear
radiance, and the RMSE in display space — the frame's and the reference's pixels through D(x) = (1 - exp(-x))^(1 / 2.2) per channel (numpy; negative
values as 0) — each beside the uniform frame's.

time: 2,040 tiles at one count on a 16 spp frame; rmd_tile_luma_error and rmd_tile_error on the same list, alternated, HIP events around the whole
synchronous call, medians of `runs` after a warm-up, min - max; rmd_tile_weighted_error under the same display table is alternated with them on the same list.

dual-table: the two rules of the dual-buffer loop at DESIGN.md section 13's set-up — both bundled scenes at 256x144, 5 bounces, 32 x 32 tiles, passes of 8,
at most 128 spp, no check below 32, against a 2,048 spp frame of seed + 1.  Settings.adaptive_denoised_threshold runs at the 30 %, 50 % and 70 % quantile
of its own measure at the first check; Settings.adaptive_denoised_display_threshold (exposure 1, gamma 2.2, floor 1 / 255) is then bisected to the threshold
whose mean samples per pixel comes closest to that point's.  Each cell: tiles stopped early, mean spp, and the RMSE of the DELIVERED (filtered) frame against
the reference, in linear radiance and in display space, each over the uniform dual-buffer frame at the mean spp rounded to a whole pass.  A display-space
RMSE under the rule's own curve favours the rule, and err sees variance and not the filter's bias: both columns are filtered frames, whose error is partly
bias no threshold on err controls.

dual-time: 2,040 tiles on a 1080p frame filtered by rmd_denoise_atrous_dual at 8 + 8 spp; rmd_tile_weighted_error_dual, rmd_tile_error_dual and
rmd_tile_weighted_error on the same list, alternated, as `time` times its calls."""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
W, H, MAX_SPP, PASS, REF_SPP, BOUNCES = 1920, 1080, 256, 16, 2048, 5
TARGETS = (245, 230, 215, 200, 180, 160)
MEASURES = ("channel_max", "luma_tile", "luma_pixel")
# ... and one that is no setting, read off the same records: sqrt(mean_variance), the tile's ABSOLUTE RMS standard error of luminance — what an RMSE in linear
# radiance is made of.  It separates "relative" from everything else the three have in common
REPLAYED = MEASURES + ("luma_absolute", "display")
DISPLAY = dict(exposure=1.0, gamma=2.2, display_floor=1.0 / 255.0)  # the tone curve the "display" measure is replayed at


def displayed(x):
    """The library's tone curve per channel at DISPLAY's exposure and gamma, before quantisation; negative values display as 0."""
    import numpy as np

    with np.errstate(invalid="ignore"):
        return (-np.expm1(-np.maximum(x, 0.0) * DISPLAY["exposure"])) ** (1.0 / DISPLAY["gamma"])


def rmse_display(a, b):
    import numpy as np

    both = np.isfinite(a) & np.isfinite(b)
    return float(np.sqrt(np.mean((displayed(a[both]) - displayed(b[both])) ** 2)))


def rmse(a, b):
    import numpy as np

    both = np.isfinite(a) & np.isfinite(b)  # (the mesh scene has a few pixels the reference's 0 x NaN makes NaN: they take no part)
    return float(np.sqrt(np.mean((a[both] - b[both]) ** 2)))


def table(a):
    import numpy as np

    from raymond_amd import lib, render, scenes
    from raymond_amd.scene import Settings, generate_tiles

    lib.load()
    scene = scenes.reflective_spheres() if a.scene == "spheres" else scenes.gold_dragon_standin()
    cam = scenes.camera(W, H)
    st = Settings(cam, sample_count=MAX_SPP, bounce_limit=BOUNCES, seed=scenes.SEED)
    tiles = generate_tiles(W, H, (32, 32))
    n_tiles, floor = len(tiles), st.adaptive_floor
    checks = list(range(PASS, MAX_SPP, PASS))  # the counts a check sees: 16 .. 240
    measures = {m: np.zeros((len(checks), n_tiles)) for m in REPLAYED}
    snapshots = []  # the sums after every pass, float64 (H, W, 3)
    weights = render.display_weights(**DISPLAY)
    result = {"display": DISPLAY, "scene": a.scene, "width": W, "height": H, "bounces": BOUNCES, "max_spp": MAX_SPP, "pass": PASS, "reference_spp": REF_SPP, "tiles": n_tiles,
              "adaptive_floor": floor, "library": os.path.relpath(lib.LIB_PATH, ROOT)}
    t0 = time.perf_counter()
    with render.Context(0) as ctx, render.DeviceScene(ctx, scene) as ds, render.Framebuffer(ctx, W, H) as fb, render.Framebuffer(ctx, W, H) as fb_sq:
        ref_st = Settings(cam, sample_count=REF_SPP, bounce_limit=BOUNCES, seed=scenes.SEED + 0x1234567)
        render.render_tiles(ctx, ds, cam, ref_st, tiles, fb, 0, REF_SPP)
        reference = fb.download() / float(REF_SPP)
        print("reference rendered, %.1f s" % (time.perf_counter() - t0), flush=True)

        def uniform(spp):
            fb.zero()
            render.render_tiles(ctx, ds, cam, st, tiles, fb, 0, spp)
            img = fb.download() / float(spp)
            return rmse(img, reference), rmse_display(img, reference)

        fb.zero()
        for k, done in enumerate(range(PASS, MAX_SPP + 1, PASS)):
            render.render_tiles(ctx, ds, cam, st, tiles, fb, done - PASS, PASS, framebuffer_sq=fb_sq)
            snapshots.append(fb.download())
            if done < MAX_SPP:
                measures["channel_max"][k] = render.tile_error(ctx, fb, fb_sq, done, floor, tiles)
                luma = render.tile_luma_error(ctx, fb, fb_sq, tiles, [done] * n_tiles, floor)
                measures["luma_tile"][k], measures["luma_pixel"][k] = luma["tile_rms"], luma["pixel_rms"]
                measures["luma_absolute"][k] = np.where(luma["invalid"] == 0, np.sqrt(luma["mean_variance"]), np.inf)
                measures["display"][k] = render.tile_weighted_error(ctx, fb, fb_sq, tiles, [done] * n_tiles, weights)["rms"]
        print("progressive render recorded, %.1f s" % (time.perf_counter() - t0), flush=True)
        result["uniform_256_rmse"] = rmse(snapshots[-1] / float(MAX_SPP), reference)
        result["uniform_256_display_rmse"] = rmse_display(snapshots[-1] / float(MAX_SPP), reference)
        result["median_at_16_spp"] = {m: float(np.median(measures[m][0])) for m in REPLAYED}
        result["median_at_240_spp"] = {m: float(np.median(measures[m][-1])) for m in REPLAYED}
        result["pixels_not_finite_at_256_spp"] = int((~np.isfinite(snapshots[-1])).any(axis=2).sum())

        def outcome(m, threshold):
            """Per tile the count it finishes with at `threshold` under measure m."""
            met = measures[m] <= threshold  # (checks, tiles)
            first = np.where(met.any(axis=0), met.argmax(axis=0), len(checks))
            return (first + 1) * PASS

        def frame_of(counts):
            img = np.empty((H, W, 3))
            for (l, t, w, h), n in zip(tiles, counts):
                img[t : t + h, l : l + w] = snapshots[n // PASS - 1][t : t + h, l : l + w] / float(n)
            return img

        rows = {m: [] for m in REPLAYED}
        uniform_cache = {}
        for m in REPLAYED:
            candidates = np.unique(measures[m][np.isfinite(measures[m])])
            for target in TARGETS:
                # the smallest recorded value whose mean spp is at or below the target: mean spp falls as the threshold rises
                lo, hi = 0, len(candidates) - 1
                while lo < hi:
                    mid = (lo + hi) // 2
                    if outcome(m, candidates[mid]).mean() <= target:
                        hi = mid
                    else:
                        lo = mid + 1
                threshold = float(candidates[lo])
                counts = outcome(m, threshold)
                mean_spp = float(counts.mean())
                spp_u = int(round(mean_spp))
                if spp_u not in uniform_cache:
                    uniform_cache[spp_u] = uniform(spp_u)
                frame = frame_of(counts)
                row = {"target_spp": target, "threshold": threshold, "tiles_stopped_early": int((counts < MAX_SPP).sum()), "mean_spp": mean_spp,
                       "rmse": rmse(frame, reference), "uniform_spp": spp_u, "uniform_rmse": uniform_cache[spp_u][0],
                       "display_rmse": rmse_display(frame, reference), "uniform_display_rmse": uniform_cache[spp_u][1]}
                row["rmse_over_uniform"] = row["rmse"] / row["uniform_rmse"]
                row["display_rmse_over_uniform"] = row["display_rmse"] / row["uniform_display_rmse"]
                rows[m].append(row)
                print("%-13s threshold %-12.6g stopped %4d  mean spp %6.1f  rmse %.6f  uniform at %3d spp %.6f  ratio %.4f  display rmse %.6f  uniform %.6f  ratio %.4f" % (
                    m, threshold, row["tiles_stopped_early"], mean_spp, row["rmse"], spp_u, row["uniform_rmse"], row["rmse_over_uniform"], row["display_rmse"],
                    row["uniform_display_rmse"], row["display_rmse_over_uniform"]), flush=True)
        result["rows"] = rows
        print("table made, %.1f s" % (time.perf_counter() - t0), flush=True)
    # one point per measure through the loop itself: the same tiles at the same counts, the same bytes
    result["loop_check"] = {}
    for m in MEASURES + ("display",):
        row = rows[m][2]
        how = dict(adaptive_display_threshold=row["threshold"], adaptive_display_exposure=DISPLAY["exposure"], adaptive_display_gamma=DISPLAY["gamma"],
                   adaptive_display_floor=DISPLAY["display_floor"]) if m == "display" else dict(adaptive_threshold=row["threshold"], adaptive_measure=m)
        loop_st = Settings(cam, sample_count=MAX_SPP, bounce_limit=BOUNCES, seed=scenes.SEED, samples_per_iteration=PASS, progress_tiles=False, **how)
        handle = render.render_tiled(scene, loop_st)
        got = {t.rect: t.sample_count for t in (msg.tile for msg in handle._messages if msg.kind == "TileFinished")}
        want = dict(zip(tiles, (int(c) for c in outcome(m, row["threshold"]))))
        same_counts = got == want
        same_bytes = handle.await_().tobytes() == frame_of(outcome(m, row["threshold"])).tobytes()
        result["loop_check"][m] = {"threshold": row["threshold"], "same_tiles_and_counts": same_counts, "same_bytes": same_bytes}
        print("loop check %-12s same tiles and counts %s, same bytes %s" % (m, same_counts, same_bytes), flush=True)
        assert same_counts and same_bytes, m
    result["seconds"] = time.perf_counter() - t0
    return result


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
        self.ok(self.rt.hipEventRecord(start, stream), "hipEventRecord")
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        self.ok(self.rt.hipEventRecord(stop, stream), "hipEventRecord")
        self.ok(self.rt.hipEventSynchronize(stop), "hipEventSynchronize")
        ms = C.c_float()
        self.ok(self.rt.hipEventElapsedTime(C.byref(ms), start, stop), "hipEventElapsedTime")
        return ms.value, wall


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "runs": len(s)}


def call_time(a):
    import numpy as np

    import tile_luma_ref
    import tile_weighted_ref
    from raymond_amd import abi, lib, render, scenes
    from raymond_amd.scene import Settings, generate_tiles, tile_array

    lib.load()
    hip = Hip()
    spp = 16
    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=BOUNCES, seed=scenes.SEED)
    tiles = generate_tiles(W, H, (32, 32))
    result = {"width": W, "height": H, "spp": spp, "tiles": len(tiles), "library": os.path.relpath(lib.LIB_PATH, ROOT),
              "how": "HIP events on the context's stream around the whole synchronous call (event), and the wall clock (wall); alternated, medians"}
    stream = hip.stream()
    with render.Context(0, stream=stream.value) as ctx, render.DeviceScene(ctx, scenes.reflective_spheres()) as ds, render.Framebuffer(ctx, W, H) as fb, \
            render.Framebuffer(ctx, W, H) as fb_sq:
        render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fb, framebuffer_sq=fb_sq)
        # held to the restatement first, on the frame's first 64 tiles
        S, Q = fb.download(), fb_sq.download()
        some = tiles[:64]
        got = render.tile_luma_error(ctx, fb, fb_sq, some, [spp] * len(some), st.adaptive_floor)
        want = tile_luma_ref.tile_luma_error(S, Q, some, [spp] * len(some), st.adaptive_floor)
        for name in ("valid", "invalid", "mean_luma", "mean_variance", "mean_rel_variance"):
            assert got[name].tobytes() == want[name].tobytes(), name
        weights = render.display_weights(**DISPLAY)
        got = render.tile_weighted_error(ctx, fb, fb_sq, some, [spp] * len(some), weights)
        want = tile_weighted_ref.tile_weighted_error(S, Q, some, [spp] * len(some), weights)
        for name in ("valid", "invalid", "mean_luma", "mean_variance", "mean_weighted_variance"):
            assert got[name].tobytes() == want[name].tobytes(), name
        arr = tile_array(tiles)
        counts = np.full(len(tiles), spp, dtype=np.uint32)
        cptr = counts.ctypes.data_as(C.POINTER(C.c_uint32))
        out_luma = np.zeros(len(tiles), dtype=render.TILE_LUMA_DTYPE)
        out_err = np.zeros(len(tiles))
        out_weighted = np.zeros(len(tiles), dtype=render.TILE_WEIGHTED_DTYPE)
        wptr = weights.ctypes.data_as(C.POINTER(C.c_double))

        def luma():
            ctx.check(ctx.L.rmd_tile_luma_error(ctx.handle, fb.ptr, fb_sq.ptr, W, H, arr, cptr, len(tiles), st.adaptive_floor, out_luma.ctypes.data_as(C.POINTER(abi.TileLuma))))

        def channel_max():
            ctx.check(ctx.L.rmd_tile_error(ctx.handle, fb.ptr, fb_sq.ptr, W, H, spp, st.adaptive_floor, arr, len(tiles), out_err.ctypes.data_as(C.c_void_p)))

        def weighted():
            ctx.check(ctx.L.rmd_tile_weighted_error(ctx.handle, fb.ptr, fb_sq.ptr, W, H, arr, cptr, len(tiles), wptr, out_weighted.ctypes.data_as(C.POINTER(abi.TileWeighted))))

        fns = {"rmd_tile_weighted_error": weighted, "rmd_tile_luma_error": luma, "rmd_tile_error": channel_max}
        for fn in fns.values():
            fn(), fn()  # warm-up: code objects, the context's scratch
        start, stop = hip.event(), hip.event()
        ev, wall = {n: [] for n in fns}, {n: [] for n in fns}
        for r in range(a.runs):
            for name in (list(fns) if r % 2 == 0 else list(reversed(fns))):  # alternated: drift falls on both alike
                e, w = hip.timed(stream, start, stop, fns[name])
                ev[name].append(e), wall[name].append(w)
        result["calls"] = {n: {"event": stats(ev[n]), "wall": stats(wall[n])} for n in fns}
        for n, v in result["calls"].items():
            print("%-22s event %.3f ms (min %.3f, max %.3f)  wall %.3f ms" % (n, v["event"]["median_ms"], v["event"]["min_ms"], v["event"]["max_ms"], v["wall"]["median_ms"]),
                  flush=True)
        result["luma_over_channel_max"] = result["calls"]["rmd_tile_luma_error"]["event"]["median_ms"] / result["calls"]["rmd_tile_error"]["event"]["median_ms"]
        result["weighted_over_luma"] = result["calls"]["rmd_tile_weighted_error"]["event"]["median_ms"] / result["calls"]["rmd_tile_luma_error"]["event"]["median_ms"]
        result["medians_of_the_frame"] = {"rmd_tile_error": float(np.median(out_err)), "tile_rms": float(np.median(out_luma["tile_rms"])),
                                          "pixel_rms": float(np.median(out_luma["pixel_rms"])), "display_rms": float(np.median(out_weighted["rms"]))}
        print(json.dumps({"luma_over_channel_max": result["luma_over_channel_max"], "weighted_over_luma": result["weighted_over_luma"],
                          "medians": result["medians_of_the_frame"]}), flush=True)
    return result


DW, DH, DSPI, DMAX, DMIN = 256, 144, 8, 128, 32  # DESIGN.md section 13's set-up


def dual_table(a):
    import numpy as np

    from raymond_amd import lib, render, scenes
    from raymond_amd.scene import Settings, generate_tiles

    lib.load()
    cam = scenes.camera(DW, DH)
    tiles = generate_tiles(DW, DH, (32, 32))
    result = {"display": DISPLAY, "width": DW, "height": DH, "bounces": BOUNCES, "max_spp": DMAX, "pass": DSPI, "adaptive_min_samples": DMIN, "reference_spp": REF_SPP,
              "tiles": len(tiles), "library": os.path.relpath(lib.LIB_PATH, ROOT), "scenes": {}}
    t0 = time.perf_counter()

    def settings(spp, **kw):
        return Settings(cam, sample_count=spp, tile_size=(32, 32), bounce_limit=BOUNCES, seed=scenes.SEED, samples_per_iteration=DSPI, denoise=True, denoise_dual=True,
                        progress_tiles=False, **kw)

    def rule(name, threshold):
        if name == "denoised":
            return dict(adaptive_denoised_threshold=threshold, adaptive_min_samples=DMIN)
        return dict(adaptive_denoised_display_threshold=threshold, adaptive_min_samples=DMIN, adaptive_display_exposure=DISPLAY["exposure"],
                    adaptive_display_gamma=DISPLAY["gamma"], adaptive_display_floor=DISPLAY["display_floor"])

    for scene_name, scene in (("spheres", scenes.reflective_spheres()), ("mesh", scenes.gold_dragon_standin(n=24))):
        with render.Context(0) as ctx, render.DeviceScene(ctx, scene) as ds, render.Framebuffer(ctx, DW, DH) as fb:
            ref_st = Settings(cam, sample_count=REF_SPP, bounce_limit=BOUNCES, seed=scenes.SEED + 1)
            render.render_tiles(ctx, ds, cam, ref_st, tiles, fb, 0, REF_SPP)
            reference = fb.download() / float(REF_SPP)

        def run(name, threshold):
            handle = render.render_tiled(scene, settings(DMAX, **rule(name, threshold)))
            done = [m.tile for m in handle._messages if m.kind == "TileFinished"]
            frame = handle.await_()
            mean_spp = sum(t.sample_count * t.width * t.height for t in done) / float(DW * DH)
            return {"threshold": threshold, "tiles_stopped_early": sum(t.sample_count < DMAX for t in done), "mean_spp": mean_spp, "rmse": rmse(frame, reference),
                    "display_rmse": rmse_display(frame, reference)}, done

        uniform_cache = {}

        def uniform(spp):
            if spp not in uniform_cache:
                frame = render.render_tiled(scene, settings(spp)).await_()
                uniform_cache[spp] = (rmse(frame, reference), rmse_display(frame, reference))
            return uniform_cache[spp]

        def against_uniform(row):
            spp_u = max(DSPI * 2, int(round(row["mean_spp"] / DSPI)) * DSPI)
            row["uniform_spp"], (row["uniform_rmse"], row["uniform_display_rmse"]) = spp_u, uniform(spp_u)
            row["rmse_over_uniform"], row["display_rmse_over_uniform"] = row["rmse"] / row["uniform_rmse"], row["display_rmse"] / row["uniform_display_rmse"]
            return row

        first = {}
        for name in ("denoised", "display"):  # the first check's measure of every tile: under a threshold everything meets every tile stops there and carries it
            probe = render.render_tiled(scene, settings(DMIN + 2 * DSPI, **rule(name, 1e300)))
            seen = np.array([np.inf if m.tile.error is None else m.tile.error for m in probe._messages if m.kind == "TileFinished"], dtype=np.float64)
            first[name] = seen[np.isfinite(seen)]  # (a tile with a pixel that is not dual-valid reads +inf and never stops: it takes no part in the quantiles)
            assert len(seen) == len(tiles) and len(first[name]) >= len(tiles) // 2
        rows = []
        for q in (0.3, 0.5, 0.7):
            row, _ = run("denoised", float(np.quantile(first["denoised"], q)))
            lo, hi = float(first["display"].min()) * 0.25, float(first["display"].max()) * 4.0
            best = None
            for _ in range(9):  # mean spp falls as the threshold rises: bisection in the logarithm
                mid = float(np.sqrt(lo * hi))
                cand, _ = run("display", mid)
                if best is None or abs(cand["mean_spp"] - row["mean_spp"]) < abs(best["mean_spp"] - row["mean_spp"]):
                    best = cand
                if cand["mean_spp"] > row["mean_spp"]:
                    lo = mid
                else:
                    hi = mid
            rows.append({"quantile": q, "denoised": against_uniform(row), "display": against_uniform(best)})
            for name in ("denoised", "display"):
                r = rows[-1][name]
                print("%-8s %-9s threshold %-12.6g stopped %3d  mean spp %6.1f  rmse %.6f  uniform at %3d spp %.6f  ratio %.4f  display rmse %.6f  uniform %.6f  ratio %.4f" % (
                    scene_name, name, r["threshold"], r["tiles_stopped_early"], r["mean_spp"], r["rmse"], r["uniform_spp"], r["uniform_rmse"], r["rmse_over_uniform"],
                    r["display_rmse"], r["uniform_display_rmse"], r["display_rmse_over_uniform"]), flush=True)
        result["scenes"][scene_name] = {"rows": rows, "first_check_median": {n: float(np.median(v)) for n, v in first.items()}}
        print(scene_name, "done, %.1f s" % (time.perf_counter() - t0), flush=True)
    result["seconds"] = time.perf_counter() - t0
    return result


def dual_call_time(a):
    import numpy as np

    import tile_weighted_dual_ref
    from raymond_amd import abi, lib, render, scenes
    from raymond_amd.scene import Settings, generate_tiles, tile_array

    lib.load()
    hip = Hip()
    half = 8
    st = Settings(scenes.camera(W, H), sample_count=2 * half, bounce_limit=BOUNCES, seed=scenes.SEED)
    tiles = generate_tiles(W, H, (32, 32))
    result = {"width": W, "height": H, "spp": 2 * half, "tiles": len(tiles), "library": os.path.relpath(lib.LIB_PATH, ROOT), "filter": "rmd_denoise_atrous_dual",
              "how": "HIP events on the context's stream around the whole synchronous call (event), and the wall clock (wall); alternated, medians"}
    stream = hip.stream()
    with contextlib.ExitStack() as stack:
        ctx = stack.enter_context(render.Context(0, stream=stream.value))
        ds = stack.enter_context(render.DeviceScene(ctx, scenes.reflective_spheres()))
        fbs = [stack.enter_context(render.Framebuffer(ctx, W, H)) for _ in range(5)]  # S_A, Q_A, S_B, Q_B, the filtered frame
        err = stack.enter_context(render.ErrorImage(ctx, W, H))
        for k in range(2):
            render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fbs[2 * k], k * half, half, framebuffer_sq=fbs[2 * k + 1])
        render.denoise_atrous_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), tiles, [half] * len(tiles), [half] * len(tiles), fbs[4], err, **st.atrous_keywords())
        weights = render.display_weights(**DISPLAY)
        # held to the restatement first, on the frame's first 64 tiles
        some = tiles[:64]
        got = render.tile_weighted_error_dual(ctx, fbs[4], err, some, weights)
        want = tile_weighted_dual_ref.tile_weighted_error_dual(fbs[4].download(), err.download(), some, weights)
        for name in ("valid", "invalid", "mean_luma", "mean_variance", "mean_weighted_variance"):
            assert got[name].tobytes() == want[name].tobytes(), name
        ones = render.tile_weighted_error_dual(ctx, fbs[4], err, tiles, np.ones(abi.LUMA_WEIGHTS))
        assert ones["rms"].tobytes() == render.tile_error_dual(ctx, err, tiles).tobytes()  # the tie, on a rendered frame
        arr = tile_array(tiles)
        counts = np.full(len(tiles), half, dtype=np.uint32)
        cptr = counts.ctypes.data_as(C.POINTER(C.c_uint32))
        out_dual, out_raw = np.zeros(len(tiles), dtype=render.TILE_WEIGHTED_DTYPE), np.zeros(len(tiles), dtype=render.TILE_WEIGHTED_DTYPE)
        out_err = np.zeros(len(tiles))
        wptr = weights.ctypes.data_as(C.POINTER(C.c_double))

        def weighted_dual():
            ctx.check(ctx.L.rmd_tile_weighted_error_dual(ctx.handle, fbs[4].ptr, err.ptr, W, H, arr, len(tiles), wptr, out_dual.ctypes.data_as(C.POINTER(abi.TileWeighted))))

        def error_dual():
            ctx.check(ctx.L.rmd_tile_error_dual(ctx.handle, err.ptr, W, H, arr, len(tiles), out_err.ctypes.data_as(C.c_void_p)))

        def weighted():
            ctx.check(ctx.L.rmd_tile_weighted_error(ctx.handle, fbs[0].ptr, fbs[1].ptr, W, H, arr, cptr, len(tiles), wptr, out_raw.ctypes.data_as(C.POINTER(abi.TileWeighted))))

        fns = {"rmd_tile_weighted_error_dual": weighted_dual, "rmd_tile_error_dual": error_dual, "rmd_tile_weighted_error": weighted}
        for fn in fns.values():
            fn(), fn()  # warm-up: code objects, the context's scratch
        start, stop = hip.event(), hip.event()
        ev, wall = {n: [] for n in fns}, {n: [] for n in fns}
        for r in range(a.runs):
            for name in (list(fns) if r % 2 == 0 else list(reversed(fns))):  # alternated: drift falls on both alike
                e, w = hip.timed(stream, start, stop, fns[name])
                ev[name].append(e), wall[name].append(w)
        result["calls"] = {n: {"event": stats(ev[n]), "wall": stats(wall[n])} for n in fns}
        for n, v in result["calls"].items():
            print("%-28s event %.3f ms (min %.3f, max %.3f)  wall %.3f ms" % (n, v["event"]["median_ms"], v["event"]["min_ms"], v["event"]["max_ms"], v["wall"]["median_ms"]),
                  flush=True)
        base = result["calls"]["rmd_tile_error_dual"]["event"]["median_ms"]
        result["weighted_dual_over_error_dual"] = result["calls"]["rmd_tile_weighted_error_dual"]["event"]["median_ms"] / base
        result["weighted_over_error_dual"] = result["calls"]["rmd_tile_weighted_error"]["event"]["median_ms"] / base
        result["bytes_read_per_pixel"] = {"rmd_tile_weighted_error_dual": 32, "rmd_tile_error_dual": 8, "rmd_tile_weighted_error": 48}
        result["medians_of_the_frame"] = {"rmd_tile_error_dual": float(np.median(out_err)), "display_rms_filtered": float(np.median(out_dual["rms"])),
                                          "display_rms_raw_half": float(np.median(out_raw["rms"]))}
        print(json.dumps({k: result[k] for k in ("weighted_dual_over_error_dual", "weighted_over_error_dual", "medians_of_the_frame")}), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("table", "time", "dual-table", "dual-time"))
    ap.add_argument("--scene", choices=("spheres", "mesh"), default="spheres")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = {"table": table, "time": call_time, "dual-table": dual_table, "dual-time": dual_call_time}[a.what](a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
