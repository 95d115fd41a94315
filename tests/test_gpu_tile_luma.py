"""rmd_tile_luma_error on the GPU against the numpy restatement (tests/tile_luma_ref.py, which tests/test_tile_luma_host.py holds to the rule header):
valid, invalid, mean_luma, mean_variance and mean_rel_variance bit for bit; tile_rms and pixel_rms, which pass through the device's square root, within
1e-12 relative — the bar tests/test_gpu_despike.py holds rmd_tile_error to —, with +inf and 0 exact.  All rects of tests/tile_luma_frames.py in one call, on
every frame class; the 300 x 300 frame's long row and column; n_rects == 0; a repeated call; the order of the sum; and Settings.adaptive_measure through
the Python loop and through raymond_cli."""
import os
import subprocess

import numpy as np
import pytest

import tile_luma_frames as frames
import tile_luma_ref as ref
from raymond_amd import render, scenes
from raymond_amd.scene import Settings, generate_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
EXACT = ("mean_luma", "mean_variance", "mean_rel_variance")
ROOTED = ("tile_rms", "pixel_rms")


def assert_device_follows(got, want, what):
    assert got.dtype == render.TILE_LUMA_DTYPE and len(got) == len(want), what
    assert list(got["valid"]) == list(want["valid"]) and list(got["invalid"]) == list(want["invalid"]), what
    for name in EXACT:
        assert ref.same_bits(got[name], want[name]), (what, name, got[name], want[name])
    for name in ROOTED:
        g, w = got[name].astype(np.float64), want[name].astype(np.float64)
        special = ~np.isfinite(w) | (w == 0.0)
        assert ref.same_bits(g[special], w[special]), (what, name, g, w)  # +inf and 0 are exact
        assert not np.isnan(g).any(), (what, name, g)
        rel = np.abs(g[~special] - w[~special]) / np.abs(w[~special])
        print(what, name, "largest relative difference", rel.max() if rel.size else 0.0)
        assert (rel <= 1e-12).all(), (what, name, g, w)


@pytest.fixture(scope="module")
def restated():
    """The restatement of every frame class, made once: name -> (S, Q, expected)."""
    rects, counts = frames.rects_and_counts(frames.RECTS)
    return {name: (S, Q, ref.tile_luma_error(S, Q, rects, counts, frames.FLOOR)) for name, (S, Q) in frames.frames().items()}


@pytest.mark.parametrize("name", ["random", "tiny", "huge", "clamped", "negative", "nan_in_S", "inf_in_Q"])
def test_every_rect_of_one_call_follows_the_restatement(gpu_ctx, restated, name):
    S, Q, want = restated[name]
    rects, counts = frames.rects_and_counts(frames.RECTS)
    got = render.tile_luma_error_arrays(gpu_ctx, S, Q, rects, counts, frames.FLOOR)
    assert_device_follows(got, want, name)
    if name in ("nan_in_S", "inf_in_Q"):
        assert got[frames.BAD_RECT]["invalid"] == 1 and got[frames.BAD_RECT]["tile_rms"] == np.inf == got[frames.BAD_RECT]["pixel_rms"]
    if name == "clamped":
        lit = [j for j, ((_, _, w, h), c) in enumerate(frames.RECTS) if w * h and c >= 2]
        assert (got["mean_variance"][lit] == 0).all() and (got["tile_rms"][lit] == 0).all()


def test_a_long_row_a_long_column_no_rects_and_a_repeated_call(gpu_ctx):
    S, Q = frames.random_positive(frames.WIDE, frames.WIDE, seed=3)
    rects, counts = frames.rects_and_counts(frames.WIDE_RECTS)
    want = ref.tile_luma_error(S, Q, rects, counts, 0.75)
    with render.Framebuffer(gpu_ctx, frames.WIDE, frames.WIDE) as fb, render.Framebuffer(gpu_ctx, frames.WIDE, frames.WIDE) as fb_sq:
        fb.upload(S), fb_sq.upload(Q)
        got = render.tile_luma_error(gpu_ctx, fb, fb_sq, rects, counts, 0.75)
        assert_device_follows(got, want, "wide")
        none = render.tile_luma_error(gpu_ctx, fb, fb_sq, [], [], 0.75)  # n_rects == 0: RMD_OK, nothing to return
        assert len(none) == 0 and none.dtype == render.TILE_LUMA_DTYPE
        again = render.tile_luma_error(gpu_ctx, fb, fb_sq, rects, counts, 0.75)  # the context's scratch block is reused
        assert got.tobytes() == again.tobytes()
        one = render.tile_luma_error(gpu_ctx, fb, fb_sq, rects[:1], counts[:1], 0.75)  # each rect is reduced on its own
        assert one.tobytes() == got[:1].tobytes()
        with pytest.raises(ValueError):
            render.tile_luma_error(gpu_ctx, fb, fb_sq, rects, counts[:1], 0.75)


def test_the_order_of_the_sum_matters_and_the_device_follows_it(gpu_ctx, restated):
    S, Q, want = restated["random"]
    rect = frames.RECTS[frames.BAD_RECT][0]
    S2, Q2 = frames.permuted_tile(S, Q, rect)
    a = ref.tile_luma_error(S, Q, [rect], [17], frames.FLOOR)
    b = ref.tile_luma_error(S2, Q2, [rect], [17], frames.FLOOR)
    assert a.tobytes() == want[frames.BAD_RECT : frames.BAD_RECT + 1].tobytes()
    assert not ref.same_bits(a["mean_variance"], b["mean_variance"])  # the same 1,024 pixels in another order: other bits
    assert_device_follows(render.tile_luma_error_arrays(gpu_ctx, S, Q, [rect], [17], frames.FLOOR), a, "as rendered")
    assert_device_follows(render.tile_luma_error_arrays(gpu_ctx, S2, Q2, [rect], [17], frames.FLOOR), b, "permuted")


# ---------------------------------------------------------------- the loop
LW, LH, LSPP, LSPI, LBOUNCES, LTILE = 64, 48, 32, 8, 3, 16
FIELD = {"luma_tile": "tile_rms", "luma_pixel": "pixel_rms"}


def loop_settings(**kw):
    return Settings(scenes.camera(LW, LH), sample_count=LSPP, tile_size=(LTILE, LTILE), bounce_limit=LBOUNCES, seed=scenes.SEED, samples_per_iteration=LSPI, **kw)


def spied_run(monkeypatch, settings):
    """render_tiled with spies on both measures: (handle, the tile_luma_error calls as (tiles, counts, result), the number of tile_error calls)."""
    luma_calls, channel_calls = [], []
    real_luma, real_channel = render.tile_luma_error, render.tile_error

    def spy_luma(ctx, framebuffer, framebuffer_sq, tiles, counts, floor):
        out = real_luma(ctx, framebuffer, framebuffer_sq, tiles, counts, floor)
        luma_calls.append((list(tiles), [int(c) for c in counts], out.copy()))
        return out

    def spy_channel(ctx, framebuffer, framebuffer_sq, sample_count, floor, tiles):
        channel_calls.append(len(tiles))
        return real_channel(ctx, framebuffer, framebuffer_sq, sample_count, floor, tiles)

    with monkeypatch.context() as patch:
        patch.setattr(render, "tile_luma_error", spy_luma)
        patch.setattr(render, "tile_error", spy_channel)
        handle = render.render_tiled(scenes.reflective_spheres(), settings)
    return handle, luma_calls, len(channel_calls)


def finished_tiles(handle):
    return {t.rect: t for t in (m.tile for m in handle._messages if m.kind == "TileFinished")}


def python_loop(monkeypatch, measure):
    """The two runs of the loop test: (threshold, first check's {rect: value}, second run's finished tiles, second run's checks)."""
    field = FIELD[measure]
    # a threshold nothing with noise meets (a tile without any variance has error 0 and meets every threshold: it is expected to stop in both runs)
    handle, calls, channel = spied_run(monkeypatch, loop_settings(adaptive_threshold=1e-300, adaptive_measure=measure))
    assert channel == 0 and len(calls) >= 1
    tiles, counts, first = calls[0]
    assert sorted(tiles) == sorted(generate_tiles(LW, LH, (LTILE, LTILE))) and len(tiles) == 12 and counts == [LSPI] * 12
    values = {rect: float(v) for rect, v in zip(tiles, first[field])}
    threshold = float(np.median(first[field]))
    assert 0.0 < threshold < np.inf
    handle, calls, channel = spied_run(monkeypatch, loop_settings(adaptive_threshold=threshold, adaptive_measure=measure))
    assert channel == 0  # render.tile_error is never called
    return threshold, values, finished_tiles(handle), calls


@pytest.mark.parametrize("measure", ["luma_tile", "luma_pixel"])
def test_the_loop_stops_exactly_the_tiles_the_measure_names(gpu_ctx, monkeypatch, measure):
    """Every figure is printed before it is asserted.  The tiles at or below the median of the first check are TileFinished at 8 samples with the spied
    value as their error.  A tile above it runs on; what becomes of it is read from the later checks' spied values in the same way — it stops at the first
    check that finds it at or below the threshold, and a tile no check finds there carries the full count."""
    field = FIELD[measure]
    threshold, values, done, calls = python_loop(monkeypatch, measure)
    print(measure, "threshold", threshold, "first check", sorted(values.values()))
    assert len(done) == 12 and sorted(done) == sorted(values)
    early = {rect for rect, v in values.items() if v <= threshold}
    assert 6 <= len(early) < 12  # the median: half of the tiles, more on ties
    for rect in early:
        assert done[rect].sample_count == LSPI and done[rect].error == values[rect], rect
    # the first check of the second run saw what the first run's saw: same seed, same pass
    assert calls[0][0] == list(values) and calls[0][2][field].tobytes() == np.array([values[r] for r in calls[0][0]]).tobytes()
    expected = {}
    for k, (tiles, counts, out) in enumerate(calls):
        assert counts == [LSPI * (k + 1)] * len(tiles) and all(r not in expected for r in tiles)  # one call per check, over the live tiles, at the pass's count
        for rect, v in zip(tiles, out[field]):
            if v <= threshold:
                expected[rect] = (LSPI * (k + 1), float(v))
    print(measure, "stopped early", {r: e for r, e in expected.items()})
    assert {r for r, (n, _) in expected.items() if n == LSPI} == early
    for rect, tile in done.items():
        if rect in expected:
            assert (tile.sample_count, tile.error) == expected[rect], rect
        else:  # the tiles that ran on to the end carry the full count
            assert tile.sample_count == LSPP and tile.error is None, rect
    assert any(t.sample_count == LSPP for t in done.values())


def test_the_default_measure_never_calls_the_luma_check(gpu_ctx, monkeypatch):
    handle, luma_calls, channel = spied_run(monkeypatch, loop_settings(adaptive_threshold=0.5))
    assert luma_calls == [] and 1 <= channel <= 3  # a check after 8, 16 and 24 samples while tiles are live
    assert len(finished_tiles(handle)) == 12
    assert loop_settings().adaptive_measure == "channel_max"


def test_cli_finishes_the_same_tiles_at_the_same_counts(gpu_ctx, monkeypatch, tmp_path):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    threshold, values, done, _ = python_loop(monkeypatch, "luma_tile")
    ppm, raw, dump = tmp_path / "o.ppm", tmp_path / "o.f64", tmp_path / "tiles.txt"
    r = subprocess.run([CLI, "render", "spheres", str(LW), str(LH), str(LSPP), str(LBOUNCES), str(ppm), "--raw", str(raw), "--spi", str(LSPI), "--tile-size", str(LTILE),
                        "--adaptive", repr(threshold), "--adaptive-measure", "luma_tile", "--dump-tiles", str(dump)], capture_output=True, text=True)
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
            assert got[rect][1] == tile.error, rect  # the measure that decided, the same bits
    assert any(n < LSPP for n, _ in got.values()) and any(n == LSPP for n, _ in got.values())
    # and so the frames are the same bytes
    handle = render.render_tiled(scenes.reflective_spheres(), loop_settings(adaptive_threshold=threshold, adaptive_measure="luma_tile"))
    handle.async_await()
    assert np.fromfile(raw).reshape(LH, LW, 3).tobytes() == handle.await_().tobytes()
