"""rmd_tile_weighted_error on the GPU against the numpy restatement (tests/tile_weighted_ref.py, which tests/test_tile_weighted_host.py holds to the rule
header): valid, invalid, mean_weighted_variance, mean_luma and mean_variance bit for bit; rms, which passes through the device's square root, within 1e-12
relative — the bar tile_rms is held to —, with +inf and 0 exact.  All rects of tests/tile_weighted_frames.py in one call, on every frame class under every
weight table; the 300 x 300 frame's long row and column; n_rects == 0; a repeated call; rmd_tile_luma_error's fields under all-ones weights; the order of
the sum; and Settings.adaptive_display_threshold through the Python loop, with a fixed and with an automatic exposure, and through raymond_cli."""
import os
import subprocess

import numpy as np
import pytest

import tile_weighted_frames as frames
import tile_weighted_ref as ref
from raymond_amd import render, scenes
from raymond_amd.scene import Settings, generate_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
EXACT = ("mean_weighted_variance", "mean_luma", "mean_variance")
FLOOR = 1.0 / 255.0


def assert_device_follows(got, want, what):
    assert got.dtype == render.TILE_WEIGHTED_DTYPE and len(got) == len(want), what
    assert list(got["valid"]) == list(want["valid"]) and list(got["invalid"]) == list(want["invalid"]), what
    for name in EXACT:
        assert ref.same_bits(got[name], want[name]), (what, name, got[name], want[name])
    g, w = got["rms"].astype(np.float64), want["rms"].astype(np.float64)
    special = ~np.isfinite(w) | (w == 0.0)
    assert ref.same_bits(g[special], w[special]), (what, "rms", g, w)  # +inf and 0 are exact
    assert not np.isnan(g).any(), (what, g)
    rel = np.abs(g[~special] - w[~special]) / np.abs(w[~special])
    print(what, "rms: largest relative difference", rel.max() if rel.size else 0.0)
    assert (rel <= 1e-12).all(), (what, g, w)


@pytest.fixture(scope="module")
def tables():
    """The weight tables, the tone curve's two from the library itself."""
    t = frames.tables()
    t["display_1"], t["display_0.001"] = render.display_weights(1.0, 2.2, FLOOR), render.display_weights(0.001, 2.2, FLOOR)
    return t


@pytest.mark.parametrize("name", ["random", "tiny", "huge", "edges", "zeros", "saturated", "nan_in_S", "inf_in_Q"])
def test_every_rect_of_one_call_follows_the_restatement_under_every_table(gpu_ctx, tables, name):
    S, Q = frames.frames()[name]
    rects, counts = frames.rects_and_counts(frames.RECTS)
    lit = [j for j, ((_, _, w, h), c) in enumerate(frames.RECTS) if w * h and c >= 2]
    with render.Framebuffer(gpu_ctx, frames.W, frames.H) as fb, render.Framebuffer(gpu_ctx, frames.W, frames.H) as fb_sq:
        fb.upload(S), fb_sq.upload(Q)
        for table_name, table in tables.items():
            got = render.tile_weighted_error(gpu_ctx, fb, fb_sq, rects, counts, table)
            assert_device_follows(got, ref.tile_weighted_error(S, Q, rects, counts, table), name + " / " + table_name)
            if name in ("nan_in_S", "inf_in_Q"):
                assert got[frames.BAD_RECT]["invalid"] == 1 and got[frames.BAD_RECT]["rms"] == np.inf
            if name == "saturated" and table_name in ("display_1", "zero", "one_bin"):  # the largest variances there are, under a zero weight
                assert ref.same_bits(got["rms"][lit], np.zeros(len(lit))) and (got["mean_variance"][lit] > 1e280).all()
            if name == "saturated" and table_name == "big":  # w * V overflows: +inf, never NaN
                assert (got["rms"][lit] == np.inf).all() and (got["invalid"][lit] == 0).all()
            if name == "random" and table_name == "one_bin":  # the lookup's index: only the pixels of that one bin count
                assert 0.0 < got[frames.BAD_RECT]["rms"] < np.inf
            if table_name == "ones":  # the two kernels share the order of the sum
                luma = render.tile_luma_error(gpu_ctx, fb, fb_sq, rects, counts, 1e-3)
                assert list(luma["valid"]) == list(got["valid"]) and list(luma["invalid"]) == list(got["invalid"])
                assert ref.same_bits(luma["mean_luma"], got["mean_luma"]) and ref.same_bits(luma["mean_variance"], got["mean_variance"])
                assert ref.same_bits(got["mean_weighted_variance"], got["mean_variance"])


def test_a_long_row_a_long_column_no_rects_and_a_repeated_call(gpu_ctx, tables):
    S, Q = frames.random_positive(frames.WIDE, frames.WIDE, seed=3)
    rects, counts = frames.rects_and_counts(frames.WIDE_RECTS)
    table = tables["random"]
    want = ref.tile_weighted_error(S, Q, rects, counts, table)
    with render.Framebuffer(gpu_ctx, frames.WIDE, frames.WIDE) as fb, render.Framebuffer(gpu_ctx, frames.WIDE, frames.WIDE) as fb_sq:
        fb.upload(S), fb_sq.upload(Q)
        got = render.tile_weighted_error(gpu_ctx, fb, fb_sq, rects, counts, table)
        assert_device_follows(got, want, "wide")
        none = render.tile_weighted_error(gpu_ctx, fb, fb_sq, [], [], table)  # n_rects == 0: RMD_OK, nothing to return
        assert len(none) == 0 and none.dtype == render.TILE_WEIGHTED_DTYPE
        again = render.tile_weighted_error(gpu_ctx, fb, fb_sq, rects, counts, table)  # the context's scratch block is reused
        assert got.tobytes() == again.tobytes()
        other = render.tile_weighted_error(gpu_ctx, fb, fb_sq, rects, counts, tables["ones"])  # ... and the weights are the call's own
        assert_device_follows(other, ref.tile_weighted_error(S, Q, rects, counts, tables["ones"]), "wide / ones")
        one = render.tile_weighted_error(gpu_ctx, fb, fb_sq, rects[:1], counts[:1], table)  # each rect is reduced on its own
        assert one.tobytes() == got[:1].tobytes()
        with pytest.raises(ValueError):
            render.tile_weighted_error(gpu_ctx, fb, fb_sq, rects, counts[:1], table)
        with pytest.raises(ValueError):
            render.tile_weighted_error(gpu_ctx, fb, fb_sq, rects, counts, table[:259])
        bad = table.copy()
        bad[259] = -1.0
        with pytest.raises(Exception, match="every weight must be finite and >= 0"):
            render.tile_weighted_error(gpu_ctx, fb, fb_sq, rects, counts, bad)


def test_the_order_of_the_sum_matters_and_the_device_follows_it(gpu_ctx, tables):
    S, Q = frames.frames()["random"]
    rect = frames.RECTS[frames.BAD_RECT][0]
    S2, Q2 = frames.permuted_tile(S, Q, rect, seed=frames.ORDER_SEED)
    for table_name in ("ones", "random"):
        table = tables[table_name]
        a = ref.tile_weighted_error(S, Q, [rect], [17], table)
        b = ref.tile_weighted_error(S2, Q2, [rect], [17], table)
        assert not ref.same_bits(a["mean_weighted_variance"], b["mean_weighted_variance"])  # the same 1,024 pixels in another order: other bits
        assert_device_follows(render.tile_weighted_error_arrays(gpu_ctx, S, Q, [rect], [17], table), a, "as rendered / " + table_name)
        assert_device_follows(render.tile_weighted_error_arrays(gpu_ctx, S2, Q2, [rect], [17], table), b, "permuted / " + table_name)


# ---------------------------------------------------------------- the loop
LW, LH, LSPP, LSPI, LBOUNCES, LTILE = 64, 48, 32, 8, 3, 16


def loop_settings(**kw):
    return Settings(scenes.camera(LW, LH), sample_count=LSPP, tile_size=(LTILE, LTILE), bounce_limit=LBOUNCES, seed=scenes.SEED, samples_per_iteration=LSPI, **kw)


def spied_run(monkeypatch, settings):
    """render_tiled with spies: (handle, the tile_weighted_error calls as (tiles, counts, weights, result), the number of tile_error calls, the
    luminance_histogram calls as (rects, counts, histogram))."""
    weighted_calls, channel_calls, histogram_calls = [], [], []
    real_weighted, real_channel, real_histogram = render.tile_weighted_error, render.tile_error, render.luminance_histogram

    def spy_weighted(ctx, framebuffer, framebuffer_sq, tiles, counts, weights):
        out = real_weighted(ctx, framebuffer, framebuffer_sq, tiles, counts, weights)
        weighted_calls.append((list(tiles), [int(c) for c in counts], np.array(weights), out.copy()))
        return out

    def spy_channel(ctx, framebuffer, framebuffer_sq, sample_count, floor, tiles):
        channel_calls.append(len(tiles))
        return real_channel(ctx, framebuffer, framebuffer_sq, sample_count, floor, tiles)

    def spy_histogram(ctx, framebuffer, rects, counts, second=None):
        out = real_histogram(ctx, framebuffer, rects, counts, second=second)
        histogram_calls.append((list(rects), [int(c) for c in counts], out))
        return out

    with monkeypatch.context() as patch:
        patch.setattr(render, "tile_weighted_error", spy_weighted)
        patch.setattr(render, "tile_error", spy_channel)
        patch.setattr(render, "luminance_histogram", spy_histogram)
        handle = render.render_tiled(scenes.reflective_spheres(), settings)
    return handle, weighted_calls, len(channel_calls), histogram_calls


def finished_tiles(handle):
    return {t.rect: t for t in (m.tile for m in handle._messages if m.kind == "TileFinished")}


def python_loop(monkeypatch, auto):
    """The two runs of the loop test: (threshold, first check's {rect: rms}, second run's finished tiles, its checks, its histograms)."""
    more = dict(adaptive_display_auto_exposure=True) if auto else {}
    # a threshold nothing with noise meets (a tile without any displayed variance has rms 0 and meets every threshold: it is expected to stop in both runs)
    handle, calls, channel, _ = spied_run(monkeypatch, loop_settings(adaptive_display_threshold=1e-300, **more))
    assert channel == 0 and len(calls) >= 1
    tiles, counts, _, first = calls[0]
    assert sorted(tiles) == sorted(generate_tiles(LW, LH, (LTILE, LTILE))) and len(tiles) == 12 and counts == [LSPI] * 12
    values = {rect: float(v) for rect, v in zip(tiles, first["rms"])}
    threshold = float(np.median(first["rms"]))
    assert 0.0 < threshold < np.inf
    handle, calls, channel, histograms = spied_run(monkeypatch, loop_settings(adaptive_display_threshold=threshold, **more))
    assert channel == 0  # render.tile_error is never called
    return threshold, values, finished_tiles(handle), calls, histograms


@pytest.mark.parametrize("auto", [False, True], ids=["fixed_exposure", "auto_exposure"])
def test_the_loop_stops_exactly_the_tiles_the_displayed_error_names(gpu_ctx, monkeypatch, auto):
    """Every figure is printed before it is asserted.  The tiles at or below the median of the first check are TileFinished at 8 samples with the spied rms
    as their error.  A tile above it runs on; it stops at the first later check that finds it at or below the threshold, and a tile no check finds there
    carries the full count.  With a fixed exposure every call's weights are rmd_display_weights' at the settings and no histogram is made; with the
    automatic exposure every check makes one histogram of the whole frame — the live tiles at the pass's count, the finished ones at theirs — and the
    call's weights are the tone curve's at the exposure that histogram asks for."""
    threshold, values, done, calls, histograms = python_loop(monkeypatch, auto)
    print("auto" if auto else "fixed", "threshold", threshold, "first check", sorted(values.values()))
    assert len(done) == 12 and sorted(done) == sorted(values)
    early = {rect for rect, v in values.items() if v <= threshold}
    assert 6 <= len(early) < 12  # the median: half of the tiles, more on ties
    for rect in early:
        assert done[rect].sample_count == LSPI and done[rect].error == values[rect], rect
    assert calls[0][0] == list(values) and calls[0][3]["rms"].tobytes() == np.array([values[r] for r in calls[0][0]]).tobytes()
    expected, stopped = {}, []
    st = loop_settings()
    assert len(histograms) == (len(calls) if auto else 0)
    for k, (tiles, counts, weights, out) in enumerate(calls):
        assert counts == [LSPI * (k + 1)] * len(tiles) and all(r not in expected for r in tiles)  # one call per check, over the live tiles, at the pass's count
        if auto:
            rects, hist_counts, hist = histograms[k]
            assert sorted(zip(rects, hist_counts)) == sorted([(r, LSPI * (k + 1)) for r in tiles] + stopped) and hist.pixels == LW * LH  # the whole frame
            exposure = render.exposure_from_histogram(hist, st.auto_exposure_percentile, st.auto_exposure_target)
            print("check", k, "exposure", exposure)
            assert ref.same_bits(weights, render.display_weights(exposure, 2.2, FLOOR)) and exposure != 1.0
        else:
            assert ref.same_bits(weights, render.display_weights(1.0, 2.2, FLOOR))
        for rect, v in zip(tiles, out["rms"]):
            if v <= threshold:
                expected[rect] = (LSPI * (k + 1), float(v))
                stopped.append((rect, LSPI * (k + 1)))
    print("stopped early", expected)
    assert {r for r, (n, _) in expected.items() if n == LSPI} == early
    for rect, tile in done.items():
        if rect in expected:
            assert (tile.sample_count, tile.error) == expected[rect], rect
        else:  # the tiles that ran on to the end carry the full count
            assert tile.sample_count == LSPP and tile.error is None, rect
    assert any(t.sample_count == LSPP for t in done.values())


def test_threshold_zero_never_calls_the_weighted_check(gpu_ctx, monkeypatch):
    handle, weighted, channel, histograms = spied_run(monkeypatch, loop_settings(adaptive_threshold=0.5))
    assert weighted == [] and histograms == [] and 1 <= channel <= 3
    handle, weighted, channel, histograms = spied_run(monkeypatch, loop_settings(adaptive_display_auto_exposure=True, adaptive_display_exposure=3.0))
    assert weighted == [] and histograms == [] and channel == 0 and len(finished_tiles(handle)) == 12  # the other display settings alone do nothing


@pytest.mark.parametrize("auto", [False, True], ids=["fixed_exposure", "auto_exposure"])
def test_cli_finishes_the_same_tiles_at_the_same_counts(gpu_ctx, monkeypatch, tmp_path, auto):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    threshold, values, done, _, _ = python_loop(monkeypatch, auto)
    ppm, raw, dump = tmp_path / "o.ppm", tmp_path / "o.f64", tmp_path / "tiles.txt"
    r = subprocess.run([CLI, "render", "spheres", str(LW), str(LH), str(LSPP), str(LBOUNCES), str(ppm), "--raw", str(raw), "--spi", str(LSPI), "--tile-size", str(LTILE),
                        "--adaptive-display", repr(threshold), "--dump-tiles", str(dump)] + (["--adaptive-display-auto-exposure", "1"] if auto else []),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = {}
    for line in dump.read_text().strip().split("\n"):
        l, t, w, h, n, e = line.split()
        got[(int(l), int(t), int(w), int(h))] = (int(n), float(e))
    print("cli", got)
    assert sorted(got) == sorted(done)
    for rect, tile in done.items():
        assert got[rect][0] == tile.sample_count, rect
        if tile.sample_count < LSPP:
            assert got[rect][1] == tile.error, rect  # the rms that decided, the same bits
    assert any(n < LSPP for n, _ in got.values()) and any(n == LSPP for n, _ in got.values())
    # and so the frames are the same bytes
    more = dict(adaptive_display_auto_exposure=True) if auto else {}
    handle = render.render_tiled(scenes.reflective_spheres(), loop_settings(adaptive_display_threshold=threshold, **more))
    handle.async_await()
    assert np.fromfile(raw).reshape(LH, LW, 3).tobytes() == handle.await_().tobytes()
