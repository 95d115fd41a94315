"""Frame previews during a progressive render (settings.preview_every, preview_denoise, progress_tiles; Message.FramePreview) on the GPU:
ReflectiveSpheres at 96 x 64 in tiles of 32, 8 spp in passes of 2, 4 bounces — through render_tiled in Python, both loops, and through raymond_cli.

A preview is checked against what the caller could have made from the messages and calls that existed before: the oracle's tone-map of the tiles a
pass's TileProgressed messages carry, rmd_denoise_atrous[_dual] + rmd_resolve_tonemap on the same samples rendered afresh."""
import os
import subprocess

import numpy as np
import pytest

from raymond_amd import render, scenes
from raymond_amd.scene import Settings, generate_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, SPI, BOUNCES = 96, 64, 8, 2, 4
TILES = generate_tiles(W, H, (32, 32))


def settings(spp=SPP, **kw):
    return Settings(scenes.camera(W, H), sample_count=spp, tile_size=(32, 32), bounce_limit=BOUNCES, samples_per_iteration=SPI, seed=scenes.SEED, **kw)


def run(st, devices=(0,)):
    """All messages of one render, in order."""
    handle = render.render_tiled(scenes.reflective_spheres(), st, devices)
    out = []
    while True:
        m = handle.poll()
        if m is None:
            return out
        out.append(m)


def tile_messages(messages, kinds=("TileProgressed", "TileFinished")):
    """What a tile message says, as comparable values: kind, rect, count, error and the bytes of its data."""
    out = []
    for m in messages:
        if m.kind in kinds:
            t = m.tile
            out.append((m.kind, t.left, t.top, t.width, t.height, t.sample_count, t.error, t.data.tobytes(), None if t.data_sq is None else t.data_sq.tobytes(),
                        None if t.data_a is None else (t.count_a, t.count_b, t.data_a.tobytes(), t.data_sq_a.tobytes(), t.data_b.tobytes(), t.data_sq_b.tobytes())))
    return out


def previews(messages):
    return [m for m in messages if m.kind == "FramePreview"]


def frame_from_tiles(oracle, tiles, exposure=1.0, gamma=2.2):
    """The oracle's tone-map of every tile at its own count, assembled."""
    frame = np.zeros((H, W, 3), dtype=np.uint8)
    for t in tiles:
        frame[t.top : t.top + t.height, t.left : t.left + t.width] = oracle.resolve_tonemap(t.data, t.sample_count, exposure, gamma)
    return frame


def progressed_by_pass(messages):
    """{sample count: the TileProgressed tiles of the pass that reached it}"""
    out = {}
    for m in messages:
        if m.kind == "TileProgressed":
            out.setdefault(m.tile.sample_count, []).append(m.tile)
    return out


@pytest.fixture(scope="module")
def default_run(gpu_ctx):
    return run(settings())


@pytest.fixture(scope="module")
def preview_run(gpu_ctx):
    return run(settings(preview_every=2))


@pytest.fixture(scope="module")
def long_preview_run(gpu_ctx):
    return run(settings(spp=12, preview_every=2))


def test_message_counts(preview_run, long_preview_run, default_run):
    """8 spp in passes of 2 are four passes, of which the fourth is the last: one preview, after pass 2.  12 spp are six: one after pass 2, one after
    pass 4, none after the last.  Each stands right behind its pass's TileProgressed messages, and all of them in front of the finished tiles."""
    assert not previews(default_run)
    for messages, n_passes in ((preview_run, 4), (long_preview_run, 6)):
        want = list(range(2, n_passes, 2))
        pv = previews(messages)
        assert [(p.pass_index, p.sample_count) for p in pv] == [(k, k * SPI) for k in want]
        assert all(p.frame.shape == (H, W, 3) and p.frame.dtype == np.uint8 and p.tile is None for p in pv)
        kinds = [m.kind for m in messages]
        n = len(TILES)
        expect = []
        for k in range(1, n_passes):
            expect += ["TileProgressed"] * n + (["FramePreview"] if k in want else [])
        assert kinds == expect + ["TileFinished"] * n


def test_tile_messages_do_not_change_with_previews_on(default_run, preview_run):
    a, b = tile_messages(default_run), tile_messages(preview_run)
    assert len(a) == len(TILES) * 4 and a == b


def test_preview_bytes_are_the_oracles_tone_map_of_that_passes_tiles(oracle, long_preview_run):
    by_pass = progressed_by_pass(long_preview_run)
    pv = previews(long_preview_run)
    assert len(pv) == 2
    for p in pv:
        tiles = by_pass[p.sample_count]
        assert len(tiles) == len(TILES)
        assert np.array_equal(p.frame, frame_from_tiles(oracle, tiles))
    other = previews(run(settings(preview_every=3, preview_exposure=0.5, preview_gamma=1.8)))  # the settings' tone-map, and another cadence: pass 3
    assert [p.pass_index for p in other] == [3]
    assert np.array_equal(other[0].frame, frame_from_tiles(oracle, progressed_by_pass(long_preview_run)[6], 0.5, 1.8))


ADAPTIVE_FLOOR = 4.0


@pytest.fixture(scope="module")
def adaptive_threshold(gpu_ctx):
    """The median rmd_tile_error of a first run, so that some tiles finish early and some do not: taken at the last count the adaptive loop checks
    (6 spp, after pass 3), and with a floor of 4.0.  At the default floor the error is a RELATIVE one of the tile's worst pixel, and at these sample
    counts every 32 x 32 tile has a pixel with a single non-zero sample — relative standard error exactly 1, the largest there is —, so all six tiles
    read the same and no threshold separates them; under a floor above the scene's radiances the error is absolute and the tiles differ."""
    st = settings()
    ds, fb, fb_sq = render.DeviceScene(gpu_ctx, scenes.reflective_spheres()), render.Framebuffer(gpu_ctx, W, H), render.Framebuffer(gpu_ctx, W, H)
    try:
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, TILES, fb, 0, SPP - SPI, framebuffer_sq=fb_sq)
        errors = render.tile_error(gpu_ctx, fb, fb_sq, SPP - SPI, ADAPTIVE_FLOOR, TILES)
        print("rmd_tile_error at %d spp:" % (SPP - SPI), sorted(float(e) for e in errors))
        return float(np.median(errors))
    finally:
        fb.close(), fb_sq.close(), ds.close()


def adaptive_settings(threshold, **kw):
    return settings(adaptive_threshold=threshold, adaptive_floor=ADAPTIVE_FLOOR, **kw)


@pytest.fixture(scope="module")
def adaptive_runs(adaptive_threshold):
    return run(adaptive_settings(adaptive_threshold)), run(adaptive_settings(adaptive_threshold, preview_every=1))


def test_adaptive_run_shows_finished_tiles_at_the_count_they_finished_with(oracle, adaptive_runs):
    plain, with_previews = adaptive_runs
    assert tile_messages(plain) == tile_messages(with_previews)
    finished = [m.tile for m in with_previews if m.kind == "TileFinished"]
    assert len(finished) == len(TILES)
    print("finished at:", sorted(t.sample_count for t in finished))
    assert any(t.sample_count < SPP for t in finished) and any(t.sample_count == SPP for t in finished)  # some finish early and some do not
    by_pass = progressed_by_pass(with_previews)
    pv = previews(with_previews)
    assert [p.pass_index for p in pv] == [1, 2, 3] and [p.sample_count for p in pv] == [2, 4, 6]
    for p in pv:
        early = [t for t in finished if t.sample_count <= p.sample_count and t.sample_count < SPP]
        live = by_pass.get(p.sample_count, [])
        assert len(early) + len(live) == len(TILES) and live
        assert np.array_equal(p.frame, frame_from_tiles(oracle, early + live))
    assert any(t.sample_count < pv[-1].sample_count for t in finished)  # a tile that finished in an earlier pass stood in a later preview


def test_without_progress_tiles_only_the_snapshots_go(default_run, preview_run, adaptive_runs, adaptive_threshold):
    quiet = run(settings(preview_every=2, progress_tiles=False))
    assert not [m for m in quiet if m.kind == "TileProgressed"]
    assert tile_messages(quiet) == tile_messages(default_run, kinds=("TileFinished",))
    assert [p.frame.tobytes() for p in previews(quiet)] == [p.frame.tobytes() for p in previews(preview_run)] and len(previews(quiet)) == 1
    # adaptive: the converged tiles' data comes through download_tiles of those tiles only — the same TileFinished messages, the same previews
    quiet = run(adaptive_settings(adaptive_threshold, preview_every=1, progress_tiles=False))
    assert not [m for m in quiet if m.kind == "TileProgressed"]
    assert tile_messages(quiet) == tile_messages(adaptive_runs[0], kinds=("TileFinished",))
    assert [p.frame.tobytes() for p in previews(quiet)] == [p.frame.tobytes() for p in previews(adaptive_runs[1])]
    # ... and with second moments in the finished tiles (denoise)
    a = run(adaptive_settings(adaptive_threshold, denoise=True))
    b = run(adaptive_settings(adaptive_threshold, denoise=True, progress_tiles=False))
    assert tile_messages(b) == tile_messages(a, kinds=("TileFinished",)) and any(t[8] is not None for t in tile_messages(b))


def test_denoised_previews_are_the_fast_filter_on_the_same_samples(gpu_ctx, default_run):
    st = settings(preview_every=2, preview_denoise=True, denoise_atrous_levels=3, denoise_atrous_k=2.0)
    messages = run(st)
    assert tile_messages(messages) == tile_messages(default_run)  # (the passes render with moments: the sums are the same)
    (p,) = previews(messages)
    done = p.sample_count
    assert done == 4
    ds = render.DeviceScene(gpu_ctx, scenes.reflective_spheres())
    fbs = [render.Framebuffer(gpu_ctx, W, H) for _ in range(3)]
    try:
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, TILES, fbs[0], 0, done, framebuffer_sq=fbs[1])  # (the bits do not depend on the split into passes)
        render.denoise_atrous(gpu_ctx, fbs[0], fbs[1], TILES, [done] * len(TILES), fbs[2], levels=3, k=2.0, alpha=st.denoise_alpha)
        want = render.resolve_tonemap(gpu_ctx, fbs[2], 1)
    finally:
        for o in fbs + [ds]:
            o.close()
    assert np.array_equal(p.frame, want)
    raw = previews(run(settings(preview_every=2)))[0].frame
    assert not np.array_equal(p.frame, raw)  # the filter did something


def test_dual_loop_previews(gpu_ctx, oracle):
    """denoise_dual: pass 1 goes to half A, pass 2 to half B; the preview after pass 2 shows a + b at n_A + n_B = 4, or rmd_denoise_atrous_dual's frame."""
    base = dict(denoise=True, denoise_dual=True)
    plain = run(settings(**base))
    raw = run(settings(preview_every=2, **base))
    den = run(settings(preview_every=2, preview_denoise=True, denoise_atrous_levels=3, **base))
    quiet = run(settings(preview_every=2, progress_tiles=False, **base))
    assert tile_messages(raw) == tile_messages(plain) and tile_messages(den) == tile_messages(plain) and not previews(plain)
    assert tile_messages(quiet) == tile_messages(plain, kinds=("TileFinished",)) and len(tile_messages(quiet)) == len(TILES)
    (p,), (pd,), (pq,) = previews(raw), previews(den), previews(quiet)
    assert (p.pass_index, p.sample_count) == (2, 4) and np.array_equal(pq.frame, p.frame)
    kinds = [m.kind for m in raw]
    assert kinds.index("FramePreview") == 2 * len(TILES)  # behind the second pass's snapshots
    st = settings(**base)
    ds = render.DeviceScene(gpu_ctx, scenes.reflective_spheres())
    fbs = [render.Framebuffer(gpu_ctx, W, H) for _ in range(5)]
    try:
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, TILES, fbs[0], 0, 2, framebuffer_sq=fbs[1])
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, TILES, fbs[2], 2, 2, framebuffer_sq=fbs[3])
        a, b = fbs[0].download(), fbs[2].download()
        assert np.array_equal(p.frame, oracle.resolve_tonemap(a + b, 4))
        render.denoise_atrous_dual(gpu_ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), TILES, [2] * len(TILES), [2] * len(TILES), fbs[4], None, levels=3,
                                   k=st.denoise_atrous_k, alpha=st.denoise_alpha)
        assert np.array_equal(pd.frame, render.resolve_tonemap(gpu_ctx, fbs[4], 1))
    finally:
        for o in fbs + [ds]:
            o.close()


def test_two_contexts_give_the_previews_of_one(preview_run, long_preview_run):
    two = run(settings(spp=12, preview_every=2), devices=(0, 0))
    assert [p.frame.tobytes() for p in previews(two)] == [p.frame.tobytes() for p in previews(long_preview_run)] and len(previews(two)) == 2
    assert [(p.pass_index, p.sample_count) for p in previews(two)] == [(2, 4), (4, 8)]


def test_async_await_hands_previews_to_their_callback():
    handle = render.render_tiled(scenes.reflective_spheres(), settings(preview_every=2))
    tiles, seen = [], []
    handle.set_callback(tiles.append)
    handle.set_preview_callback(seen.append)
    handle.async_await()
    assert len(tiles) == 3 * len(TILES) and [m.pass_index for m in seen] == [2] and seen[0].kind == "FramePreview"
    image = handle.await_()  # the finished tiles are what is left: await_ is unchanged
    assert image.shape == (H, W, 3) and np.isfinite(image).all() and image.any()


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")


def read_ppm(path):
    with open(path, "rb") as f:
        assert f.readline() == b"P6\n" and f.readline() == b"%d %d\n" % (W, H) and f.readline() == b"255\n"
        return np.frombuffer(f.read(), dtype=np.uint8).reshape(H, W, 3)


def test_cli_writes_the_python_previews(cli, tmp_path, long_preview_run):
    def render_cli(name, spp, *flags):
        prefix = tmp_path / name
        r = subprocess.run([cli, "render", "spheres", str(W), str(H), str(spp), str(BOUNCES), str(tmp_path / (name + ".ppm")), "--spi", str(SPI), "--preview-every", "2",
                            "--preview-prefix", str(prefix)] + [str(f) for f in flags], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return sorted(p.name for p in tmp_path.glob(name + "_*.ppm")), prefix

    names, prefix = render_cli("raw", 12)
    assert names == ["raw_0001.ppm", "raw_0002.ppm"]
    for k, p in enumerate(previews(long_preview_run)):
        assert np.array_equal(read_ppm("%s_%04d.ppm" % (prefix, k + 1)), p.frame)
    names, prefix = render_cli("den", SPP, "--preview-denoise", 1, "--progress-tiles", 0, "--denoise-atrous-levels", 3)
    assert names == ["den_0001.ppm"]
    (p,) = previews(run(settings(preview_every=2, preview_denoise=True, progress_tiles=False, denoise_atrous_levels=3)))
    assert np.array_equal(read_ppm("%s_0001.ppm" % prefix), p.frame)
    names, prefix = render_cli("dual", SPP, "--denoise", 1, "--denoise-dual", 1)
    assert names == ["dual_0001.ppm"]
    (p,) = previews(run(settings(preview_every=2, denoise=True, denoise_dual=True)))
    assert np.array_equal(read_ppm("%s_0001.ppm" % prefix), p.frame)
    # the dual loop's filtered preview: rmd_denoise_atrous_dual on the two halves ...
    names, prefix = render_cli("dualden", SPP, "--denoise", 1, "--denoise-dual", 1, "--preview-denoise", 1)
    assert names == ["dualden_0001.ppm"]
    (p,) = previews(run(settings(preview_every=2, denoise=True, denoise_dual=True, preview_denoise=True)))
    assert np.array_equal(read_ppm("%s_0001.ppm" % prefix), p.frame)
    # ... and guided: a threshold no tile reaches makes the loop keep the feature buffers, which the preview's filter then reads
    names, prefix = render_cli("dualguided", SPP, "--denoise", 1, "--denoise-dual", 1, "--preview-denoise", 1, "--denoise-dual-features", 1, "--adaptive-denoised", "1e-9",
                               "--adaptive-min", 2)
    assert names == ["dualguided_0001.ppm"]
    (p,) = previews(run(settings(preview_every=2, denoise=True, denoise_dual=True, preview_denoise=True, denoise_dual_features=True, adaptive_denoised_threshold=1e-9,
                                 adaptive_min_samples=2)))
    assert np.array_equal(read_ppm("%s_0001.ppm" % prefix), p.frame)
    r = subprocess.run([cli, "render", "spheres", str(W), str(H), str(SPP), str(BOUNCES), str(tmp_path / "x.ppm"), "--preview-every", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "preview_every > 0 needs samples_per_iteration > 0" in r.stderr  # the settings' rule, in the C++ mirror's words too
