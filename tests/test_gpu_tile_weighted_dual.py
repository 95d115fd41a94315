"""rmd_tile_weighted_error_dual on the GPU against the numpy restatement (tests/tile_weighted_dual_ref.py, which tests/test_tile_weighted_dual_host.py holds
to the rule header): valid, invalid, mean_weighted_variance, mean_luma and mean_variance bit for bit; rms, which passes through the device's square root, as
tests/test_gpu_tile_weighted.py's assert_device_follows holds it — within 1e-12 relative of the root of the radicand the device itself reports bit for bit,
with +inf and 0 exact.  All rects of tests/tile_weighted_dual_frames.py in one call, on every frame class under every weight table; the 300 x 300 frame's
long row and column; n_rects == 0; a repeated call; the order of the sum; the tie with rmd_tile_error_dual under all-ones weights; and
Settings.adaptive_denoised_display_threshold through the Python loop — default and a-trous filter, fixed and automatic exposure — and through raymond_cli."""
import os
import subprocess

import numpy as np
import pytest

import tile_weighted_dual_frames as frames
import tile_weighted_dual_ref as ref
from raymond_amd import render, scenes
from raymond_amd.scene import Settings, generate_tiles
from test_gpu_tile_weighted import assert_device_follows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
FLOOR = 1.0 / 255.0
FRAME_NAMES = ["random", "tiny", "huge", "edges", "zeros", "inf_err", "nan_err", "nan_out", "inf_out", "negative_err"]


@pytest.fixture(scope="module")
def tables():
    """The weight tables, the tone curve's two from the library itself."""
    t = frames.tables()
    t["display_1"], t["display_0.001"] = render.display_weights(1.0, 2.2, FLOOR), render.display_weights(0.001, 2.2, FLOOR)
    return t


class Uploaded:
    """An (out, err) pair in a framebuffer and an error image."""

    def __init__(self, ctx, out, err):
        self.ctx, (self.h, self.w) = ctx, err.shape
        self.out, self.err = out, err

    def __enter__(self):
        self.fb, self.img = render.Framebuffer(self.ctx, self.w, self.h), render.ErrorImage(self.ctx, self.w, self.h)
        self.fb.upload(self.out), self.img.upload(self.err)
        return self.fb, self.img

    def __exit__(self, *exc):
        self.img.close(), self.fb.close()


@pytest.mark.parametrize("name", FRAME_NAMES)
def test_every_rect_of_one_call_follows_the_restatement_under_every_table(gpu_ctx, tables, name):
    out, err = frames.frames()[name]
    rects = frames.RECTS
    lit = [j for j, (_, _, w, h) in enumerate(rects) if w * h > 1]  # (the one-pixel rect holds no pixel of the every-fourth classes)
    with Uploaded(gpu_ctx, out, err) as (fb, img):
        for table_name, table in tables.items():
            got = render.tile_weighted_error_dual(gpu_ctx, fb, img, rects, table)
            want = ref.tile_weighted_error_dual(out, err, rects, table)
            assert_device_follows(got, want, name + " / " + table_name)
            if name in frames.INVALID_CLASSES:
                bad = got[frames.BAD_RECT]
                assert bad["invalid"] == 1 and bad["valid"] == 1023 and bad["rms"] == np.inf and 0 < bad["mean_luma"] < np.inf
                assert [j for j in range(len(rects)) if got[j]["invalid"]] == [frames.BAD_RECT]
            if name == "inf_err":
                assert not any(np.isnan(got[f]).any() for f in ref.FLOAT_FIELDS) and (got["invalid"] == 0).all() and (got["mean_variance"][lit] == np.inf).all()
                if table_name == "zero":  # w = 0 under e = +inf adds 0
                    assert ref.same_bits(got["rms"][lit], np.zeros(len(lit)))
                if table_name == "big":
                    assert (got["rms"][lit] == np.inf).all()
                if table_name == "one_bin":  # the infinite pixels lie outside that bin
                    assert np.isfinite(got["rms"]).all() and got[frames.TILE_RECT]["rms"] > 0.0
            if name == "negative_err" and table_name == "ones":
                neg = got[frames.NEG_RECT]
                assert neg["mean_weighted_variance"] < 0 and neg["rms"] == np.inf and neg["invalid"] == 0
            if name == "random" and table_name == "one_bin":  # the lookup's index: only the pixels of that one bin count
                assert 0.0 < got[frames.TILE_RECT]["rms"] < np.inf


def test_a_long_row_a_long_column_no_rects_and_a_repeated_call(gpu_ctx, tables):
    out, err = frames.wide_frame()
    rects, table = frames.WIDE_RECTS, tables["random"]
    want = ref.tile_weighted_error_dual(out, err, rects, table)
    with Uploaded(gpu_ctx, out, err) as (fb, img):
        got = render.tile_weighted_error_dual(gpu_ctx, fb, img, rects, table)
        assert_device_follows(got, want, "wide")
        none = render.tile_weighted_error_dual(gpu_ctx, fb, img, [], table)  # n_rects == 0: RMD_OK, nothing to return
        assert len(none) == 0 and none.dtype == render.TILE_WEIGHTED_DTYPE
        again = render.tile_weighted_error_dual(gpu_ctx, fb, img, rects, table)  # the context's scratch block is reused
        assert got.tobytes() == again.tobytes()
        other = render.tile_weighted_error_dual(gpu_ctx, fb, img, rects, tables["ones"])  # ... and the weights are the call's own
        assert_device_follows(other, ref.tile_weighted_error_dual(out, err, rects, tables["ones"]), "wide / ones")
        one = render.tile_weighted_error_dual(gpu_ctx, fb, img, rects[:1], table)  # each rect is reduced on its own
        assert one.tobytes() == got[:1].tobytes()
        with pytest.raises(ValueError):
            render.tile_weighted_error_dual(gpu_ctx, fb, img, rects, table[:259])
        bad = table.copy()
        bad[259] = -1.0
        with pytest.raises(Exception, match="every weight must be finite and >= 0"):
            render.tile_weighted_error_dual(gpu_ctx, fb, img, rects, bad)
        with pytest.raises(Exception, match="err_dev must not alias out_dev"):
            render.tile_weighted_error_dual(gpu_ctx, fb, fb, rects, table)


def test_the_order_of_the_sum_matters_and_the_device_follows_it(gpu_ctx, tables):
    out, err = frames.frames()["random"]
    rect = frames.RECTS[frames.TILE_RECT]
    out2, err2 = frames.permuted(out, err, rect, seed=frames.ORDER_SEED)
    with Uploaded(gpu_ctx, out, err) as (fb, img), Uploaded(gpu_ctx, out2, err2) as (fb2, img2):
        for table_name in ("ones", "random"):
            table = tables[table_name]
            a = ref.tile_weighted_error_dual(out, err, [rect], table)
            b = ref.tile_weighted_error_dual(out2, err2, [rect], table)
            assert not ref.same_bits(a["mean_weighted_variance"], b["mean_weighted_variance"])  # the same 1,024 pixels in another order: other bits
            assert_device_follows(render.tile_weighted_error_dual(gpu_ctx, fb, img, [rect], table), a, "as made / " + table_name)
            assert_device_follows(render.tile_weighted_error_dual(gpu_ctx, fb2, img2, [rect], table), b, "permuted / " + table_name)


@pytest.mark.parametrize("name", ["random", "tiny", "huge", "inf_err", "nan_err"])
def test_all_ones_weights_give_rmd_tile_error_duals_result_bit_for_bit(gpu_ctx, tables, name):
    out, err = frames.frames()[name]
    rects = frames.RECTS
    with Uploaded(gpu_ctx, out, err) as (fb, img):
        got = render.tile_weighted_error_dual(gpu_ctx, fb, img, rects, tables["ones"])
        plain = render.tile_error_dual(gpu_ctx, img, rects)
    print(name, "rms", got["rms"], "rmd_tile_error_dual", plain)
    if name == "nan_err":
        assert got[frames.BAD_RECT]["rms"] == np.inf and plain[frames.BAD_RECT] == np.inf
    assert (got["invalid"] == 0).sum() == len(rects) - (name == "nan_err")
    assert ref.same_bits(got["rms"], plain)  # every rect: the same lanes, the same combine, the same square root
    assert ref.same_bits(got["mean_variance"], got["mean_weighted_variance"])
    assert ref.same_bits(got["mean_variance"][got["invalid"] == 0], ref.tile_error_dual(err, rects)[1][got["invalid"] == 0])  # ... and mean_variance is its radicand


# ---------------------------------------------------------------- the loop
LW, LH, LSPP, LSPI, LBOUNCES, LTILE, LMIN = 64, 48, 48, 8, 3, 16, 16
CHECKS = (16, 32)  # the even passes that leave live tiles below LSPP with at least LMIN samples
EXPOSURE = 1.5  # the fixed exposure: not the default, so that the settings are seen to be read


def loop_settings(**kw):
    return Settings(scenes.camera(LW, LH), sample_count=LSPP, tile_size=(LTILE, LTILE), bounce_limit=LBOUNCES, seed=scenes.SEED, samples_per_iteration=LSPI, denoise=True,
                    denoise_dual=True, adaptive_min_samples=LMIN, **kw)


def display_settings(threshold, atrous, auto):
    more = dict(adaptive_display_auto_exposure=True) if auto else dict(adaptive_display_exposure=EXPOSURE)
    return loop_settings(adaptive_denoised_display_threshold=threshold, denoise_dual_atrous=atrous, **more)


def spied_run(monkeypatch, settings):
    """render_tiled with spies: (handle, the tile_weighted_error_dual calls as (tiles, weights, result, the two buffers' addresses), the number of
    tile_error_dual calls, the luminance_histogram calls as (rects, counts, histogram, the two buffers' addresses))."""
    weighted_calls, plain_calls, histogram_calls = [], [], []
    real_weighted, real_plain, real_histogram = render.tile_weighted_error_dual, render.tile_error_dual, render.luminance_histogram

    def spy_weighted(ctx, out_fb, err_img, tiles, weights):
        out = real_weighted(ctx, out_fb, err_img, tiles, weights)
        weighted_calls.append((list(tiles), np.array(weights), out.copy(), (out_fb.ptr.value, err_img.ptr.value)))
        return out

    def spy_plain(ctx, error_image, tiles):
        plain_calls.append(len(tiles))
        return real_plain(ctx, error_image, tiles)

    def spy_histogram(ctx, framebuffer, rects, counts, second=None):
        out = real_histogram(ctx, framebuffer, rects, counts, second=second)
        histogram_calls.append((list(rects), [int(c) for c in counts], out, (framebuffer.ptr.value, None if second is None else second.ptr.value)))
        return out

    with monkeypatch.context() as patch:
        patch.setattr(render, "tile_weighted_error_dual", spy_weighted)
        patch.setattr(render, "tile_error_dual", spy_plain)
        patch.setattr(render, "luminance_histogram", spy_histogram)
        handle = render.render_tiled(scenes.reflective_spheres(), settings)
    return handle, weighted_calls, len(plain_calls), histogram_calls


def finished_tiles(handle):
    return {t.rect: t for t in (m.tile for m in handle._messages if m.kind == "TileFinished")}


_LOOPS = {}


def python_loop(monkeypatch, atrous, auto):
    """The two runs of the loop test, made once per variant: (threshold, first check's {rect: rms}, second run's finished tiles, its checks, its histograms)."""
    if (atrous, auto) not in _LOOPS:
        # a threshold nothing with noise meets: the first check's rms of every tile
        handle, calls, plain, _ = spied_run(monkeypatch, display_settings(1e-300, atrous, auto))
        assert plain == 0 and len(calls) >= 1
        tiles, _, first, _ = calls[0]
        assert tiles == generate_tiles(LW, LH, (LTILE, LTILE)) and len(tiles) == 12
        values = {rect: float(v) for rect, v in zip(tiles, first["rms"])}
        threshold = float(np.median(first["rms"]))
        assert 0.0 < threshold < np.inf
        handle, calls, plain, histograms = spied_run(monkeypatch, display_settings(threshold, atrous, auto))
        assert plain == 0  # render.tile_error_dual is never called
        _LOOPS[(atrous, auto)] = threshold, values, finished_tiles(handle), calls, histograms
    return _LOOPS[(atrous, auto)]


@pytest.mark.parametrize("auto", [False, True], ids=["fixed_exposure", "auto_exposure"])
@pytest.mark.parametrize("atrous", [False, True], ids=["default_filter", "atrous"])
def test_the_loop_stops_exactly_the_tiles_the_filtered_frames_displayed_error_names(gpu_ctx, monkeypatch, atrous, auto):
    """Every figure is printed before it is asserted.  The tiles at or below the median of the first check are TileFinished at 16 samples with the spied rms
    as their error.  A tile above it runs on; it stops at the check at 32 samples if that finds it at or below the threshold, and a tile no check finds
    there carries the full count.  With a fixed exposure every call's weights are rmd_display_weights' at the settings and no histogram is made; with the
    automatic exposure every check makes one histogram of the whole frame on the raw halves — the live tiles at n_A + n_B, the finished ones at theirs —
    and the call's weights are the tone curve's at the exposure that histogram asks for."""
    threshold, values, done, calls, histograms = python_loop(monkeypatch, atrous, auto)
    print("atrous" if atrous else "default", "auto" if auto else "fixed", "threshold", threshold, "first check", sorted(values.values()))
    assert len(done) == 12 and sorted(done) == sorted(values)
    early = {rect for rect, v in values.items() if v <= threshold}
    assert 6 <= len(early) < 12  # the median: half of the tiles, more on ties — a condition of the median, not a measurement
    for rect in early:
        assert done[rect].sample_count == CHECKS[0] and done[rect].error == values[rect] and (done[rect].count_a, done[rect].count_b) == (8, 8), rect
    assert calls[0][0] == list(values) and calls[0][2]["rms"].tobytes() == np.array([values[r] for r in calls[0][0]]).tobytes()
    expected, stopped = {}, []
    st = loop_settings()
    assert 1 <= len(calls) <= len(CHECKS) and len(histograms) == (len(calls) if auto else 0)
    for k, (tiles, weights, out, (out_at, err_at)) in enumerate(calls):
        assert tiles == [r for r in generate_tiles(LW, LH, (LTILE, LTILE)) if r not in expected]  # one call per check, over exactly the live tiles
        if auto:
            rects, hist_counts, hist, (first_at, second_at) = histograms[k]
            assert sorted(zip(rects, hist_counts)) == sorted([(r, CHECKS[k]) for r in tiles] + stopped) and hist.pixels == LW * LH  # the whole frame, at the stated counts
            assert second_at is not None and len({first_at, second_at, out_at, err_at}) == 4  # two buffers, neither of them the filtered frame
            exposure = render.exposure_from_histogram(hist, st.auto_exposure_percentile, st.auto_exposure_target)
            print("check", k, "exposure", exposure)
            assert ref.same_bits(weights, render.display_weights(exposure, 2.2, FLOOR)) and exposure != 1.0
        else:
            assert ref.same_bits(weights, render.display_weights(EXPOSURE, 2.2, FLOOR)) and not ref.same_bits(weights, render.display_weights(1.0, 2.2, FLOOR))
        for rect, v in zip(tiles, out["rms"]):
            if v <= threshold:
                expected[rect] = (CHECKS[k], float(v))
                stopped.append((rect, CHECKS[k]))
    print("stopped early", expected)
    assert {r for r, (n, _) in expected.items() if n == CHECKS[0]} == early
    for rect, tile in done.items():
        if rect in expected:
            assert (tile.sample_count, tile.error) == expected[rect], rect
        else:  # the tiles that ran on to the end carry the full count
            assert tile.sample_count == LSPP and tile.error is None, rect
    assert 6 <= len(expected) < 12 and any(t.sample_count == LSPP for t in done.values())


def test_threshold_zero_never_calls_the_weighted_check(gpu_ctx, monkeypatch):
    handle, weighted, plain, histograms = spied_run(monkeypatch, loop_settings(adaptive_denoised_threshold=1e-300, adaptive_display_auto_exposure=True, adaptive_display_exposure=3.0))
    assert weighted == [] and histograms == [] and plain == len(CHECKS) and len(finished_tiles(handle)) == 12  # the other display settings alone do nothing
    handle, weighted, plain, histograms = spied_run(monkeypatch, loop_settings())
    assert weighted == [] and histograms == [] and plain == 0 and len(finished_tiles(handle)) == 12


@pytest.mark.parametrize("auto", [False, True], ids=["fixed_exposure", "auto_exposure"])
def test_cli_finishes_the_same_tiles_at_the_same_counts(gpu_ctx, monkeypatch, tmp_path, auto):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    threshold, values, done, _, _ = python_loop(monkeypatch, False, auto)
    ppm, raw, dump = tmp_path / "o.ppm", tmp_path / "o.f64", tmp_path / "tiles.txt"
    r = subprocess.run([CLI, "render", "spheres", str(LW), str(LH), str(LSPP), str(LBOUNCES), str(ppm), "--raw", str(raw), "--spi", str(LSPI), "--tile-size", str(LTILE),
                        "--denoise", "1", "--denoise-dual", "1", "--adaptive-denoised-display", repr(threshold), "--adaptive-min", str(LMIN), "--dump-tiles", str(dump)]
                       + (["--adaptive-display-auto-exposure", "1"] if auto else ["--adaptive-display-exposure", repr(EXPOSURE)]), capture_output=True, text=True)
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
    handle = render.render_tiled(scenes.reflective_spheres(), display_settings(threshold, False, auto))
    handle.async_await()
    assert np.fromfile(raw).reshape(LH, LW, 3).tobytes() == handle.await_().tobytes()
