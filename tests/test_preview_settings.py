"""Settings.check_preview's rules and render.scatter_tiles, without a GPU."""
import numpy as np
import pytest

from raymond_amd import render, scenes
from raymond_amd.scene import Settings


def settings(**kw):
    return Settings(scenes.camera(96, 64), 8, **kw)


def test_the_defaults_are_off_and_pass():
    st = settings()
    assert st.preview_every == 0 and st.preview_exposure == 1.0 and st.preview_gamma == 2.2 and st.preview_denoise is False and st.progress_tiles is True
    st.check_preview()
    st.check_preview(2)
    on = settings(samples_per_iteration=2, preview_every=2, preview_denoise=True, progress_tiles=False, preview_exposure=0.5, preview_gamma=1.8)
    on.check_preview()
    assert (on.preview_every, on.preview_exposure, on.preview_gamma, on.preview_denoise, on.progress_tiles) == (2, 0.5, 1.8, True, False)


def test_preview_every_needs_progressive_passes():
    with pytest.raises(ValueError, match="preview_every > 0 needs samples_per_iteration > 0"):
        settings(preview_every=2)
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="preview_every must be an integer >= 0"):
            settings(samples_per_iteration=2, preview_every=bad)


def test_preview_denoise_needs_previews():
    with pytest.raises(ValueError, match="preview_denoise needs preview_every > 0"):
        settings(samples_per_iteration=2, preview_denoise=True)


def test_preview_denoise_is_refused_on_two_devices():
    st = settings(samples_per_iteration=2, preview_every=1, preview_denoise=True)
    st.check_preview(1)
    with pytest.raises(ValueError, match="preview_denoise renders on one device: the filter's window crosses the tiles that several devices would own"):
        st.check_preview(2)
    settings(samples_per_iteration=2, preview_every=1).check_preview(2)  # raw previews: every device resolves its share
    with pytest.raises(ValueError, match="renders on one device"):  # ... and render_tiled asks before it opens a device
        render.render_tiled(scenes.reflective_spheres(), st, devices=(0, 0))


@pytest.mark.parametrize("name", ["preview_exposure", "preview_gamma"])
@pytest.mark.parametrize("bad", [0.0, -1.0, float("inf"), float("nan")])
def test_the_tone_map_of_the_previews_is_finite_and_positive(name, bad):
    with pytest.raises(ValueError, match=name + " must be finite and > 0"):
        settings(**{name: bad})


def test_scatter_tiles_on_ragged_rects():
    rng = np.random.default_rng(5)
    W, H = 23, 17
    rects = [(0, 0, 1, 1), (22, 16, 1, 1), (3, 2, 7, 5), (0, 9, 23, 1), (11, 0, 1, 17), (5, 5, 0, 3), (6, 6, 4, 0), (16, 10, 7, 7)]
    tiles = [rng.integers(1, 256, (h, w, 3), dtype=np.uint8) for (_, _, w, h) in rects]
    want = np.zeros((H, W, 3), dtype=np.uint8)
    for (l, t, w, h), d in zip(rects, tiles):
        for y in range(h):
            for x in range(w):
                want[t + y, l + x] = d[y, x]  # in order: a later rect overwrites an earlier one where they overlap
    got = render.scatter_tiles(rects, tiles, W, H)
    assert got.dtype == np.uint8 and got.shape == (H, W, 3) and np.array_equal(got, want)
    assert (got[14, 2] == 0).all()  # a pixel no rect covers stays zero
    # flat views of one packed block, as resolve_tonemap_tiles returns them, into a frame of the caller's
    packed = np.concatenate([d.reshape(-1) for d in tiles])
    views, at = [], 0
    for (_, _, w, h) in rects:
        views.append(packed[at : at + w * h * 3].reshape(h, w, 3))
        at += w * h * 3
    frame = np.full((H, W, 3), 9, dtype=np.uint8)
    assert render.scatter_tiles(rects, views, out=frame) is frame
    covered = np.zeros((H, W), dtype=bool)
    for (l, t, w, h) in rects:
        covered[t : t + h, l : l + w] = True
    assert np.array_equal(frame[covered], want[covered]) and (frame[~covered] == 9).all()
    # float64 tiles (download_tiles's) keep their dtype
    f64 = render.scatter_tiles([(1, 1, 2, 2)], [np.arange(12.0).reshape(2, 2, 3)], 4, 4)
    assert f64.dtype == np.float64 and f64[2, 2, 2] == 11.0 and f64[0, 0, 0] == 0.0
    with pytest.raises(ValueError, match="outside"):
        render.scatter_tiles([(20, 0, 4, 1)], [np.zeros((1, 4, 3), np.uint8)], W, H)
    with pytest.raises(ValueError, match="one array per rect"):
        render.scatter_tiles(rects, tiles[:-1], W, H)
    with pytest.raises(ValueError, match="needs a frame"):
        render.scatter_tiles(rects, tiles)
