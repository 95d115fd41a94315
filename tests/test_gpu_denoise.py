"""rmd_denoise on the device: the kernel against the numpy restatement (tests/denoise_ref.py), its exact properties, its quality on real
renders, and the host paths that use it (Python render_tiled / await_, the C++ mirror through raymond_cli)."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref
from raymond_amd import render, scenes
from raymond_amd.scene import Settings, generate_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")


def _tiles_with_counts(W, H, tw, th, rng, uncovered=True):
    """A tiling of the frame with a sample count per tile (2 .. 64, some 1 and 0), and one tile left out when `uncovered`."""
    rects = generate_tiles(W, H, (tw, th))
    counts = [int(c) for c in rng.integers(2, 65, len(rects))]
    if len(rects) >= 4:
        counts[1], counts[2] = 1, 0
    if uncovered and len(rects) >= 3:
        del rects[-2], counts[-2]
    return rects, counts


def _moments(rng, n_img):
    """Sums and sums of squares of n samples per pixel (a smooth image plus noise whose level varies over the frame)."""
    H, W = n_img.shape
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([0.5 + 0.4 * np.sin(x / 5.0), 0.3 + 0.2 * np.cos(y / 3.0), 0.2 + 0.1 * ((x + y) % 7)], axis=-1)
    sigma = rng.uniform(0.0, 0.6, (H, W, 1)) * (1 + (x % 9 == 0))[..., None]
    n = np.maximum(n_img, 0).astype(np.float64)[..., None]
    mean = base + rng.normal(0.0, 1.0, (H, W, 3)) * sigma / np.sqrt(np.maximum(n, 1.0))
    S = mean * n
    Q = S * mean + rng.uniform(0.0, 1.0, (H, W, 3)) * sigma * sigma * np.maximum(n - 1.0, 0.0)
    Q[rng.uniform(size=(H, W, 3)) < 0.02] *= 0.5  # some below S^2 / n: a negative variance estimate, clamped to 0
    return S, Q


def _poison(S, Q, rng):
    """NaN and inf in S, inf in Q, at a few pixels."""
    H, W = S.shape[:2]
    for value, arr in ((np.nan, S), (np.inf, S), (-np.inf, S), (np.inf, Q)):
        for _ in range(max(1, H * W // 400)):
            arr[rng.integers(0, H), rng.integers(0, W), rng.integers(0, 3)] = value


def _agree(dev, ref):
    """Within 1e-9 relative plus 1e-12 of the frame's largest |u|; NaN exactly where the restatement has NaN; infinities equal."""
    fin = np.isfinite(ref)
    scale = np.max(np.abs(ref[fin])) if fin.any() else 0.0
    assert np.array_equal(np.isnan(dev), np.isnan(ref))
    assert np.array_equal(dev[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    err = np.abs(dev[fin] - ref[fin])
    bad = err > 1e-9 * np.abs(ref[fin]) + 1e-12 * scale
    assert not bad.any(), "%d values differ, worst %.3g" % (bad.sum(), err.max())


CASES = [(0, 0, 0.45, 1.0), (1, 0, 0.45, 1.0), (3, 1, 0.3, 0.5), (10, 3, 0.45, 1.0), (12, 4, 1.0, 0.0), (3, 1, 2.0, 4.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1, 1), (5, 200), (37, 23), (64, 48)])
def test_kernel_matches_the_restatement(gpu_ctx, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    rects, counts = _tiles_with_counts(W, H, 8, 16, rng) if W * H > 1 else ([(0, 0, 1, 1)], [9])
    n_img = denoise_ref.count_image(W, H, rects, counts)
    S, Q = _moments(rng, n_img)
    if W * H > 1:
        _poison(S, Q, rng)
    for r, f, k, alpha in CASES:
        dev = render.denoise_arrays(gpu_ctx, S, Q, rects, counts, radius=r, patch_radius=f, k=k, alpha=alpha)
        ref = denoise_ref.denoise(S, Q, n_img, radius=r, patch_radius=f, k=k, alpha=alpha)
        _agree(dev, ref)


def _plain_frame(rng, W, H, n):
    n_img = np.full((H, W), n)
    S, Q = _moments(rng, n_img)
    return S, Q, [(0, 0, W, H)], [n]


@pytest.mark.gpu
def test_radius_zero_is_the_mean_bit_for_bit(gpu_ctx):
    rng = np.random.default_rng(3)
    W, H = 45, 29
    rects, counts = _tiles_with_counts(W, H, 16, 8, rng)
    n_img = denoise_ref.count_image(W, H, rects, counts)
    S, Q = _moments(rng, n_img)
    _poison(S, Q, rng)
    S[3, 3] = -0.0  # -0.0 / n stays -0.0
    with np.errstate(all="ignore"):
        mean = S / n_img[..., None].astype(np.float64)
    for f in (0, 1, 4):
        out = render.denoise_arrays(gpu_ctx, S, Q, rects, counts, radius=0, patch_radius=f)
        assert out.tobytes() == mean.tobytes()


@pytest.mark.gpu
def test_zero_variance_dyadic_frame_comes_back_bit_for_bit(gpu_ctx):
    rng = np.random.default_rng(4)
    W, H, n = 70, 41, 8
    u = rng.integers(0, 8, (H, W, 3)) * 0.25
    u[10:20, 10:30] = 0.5  # flat regions: many neighbours with weight 1
    S = u * n
    Q = S * u
    for r, f in ((1, 0), (3, 1), (10, 3), (12, 4)):
        out = render.denoise_arrays(gpu_ctx, S, Q, [(0, 0, W, H)], [n], radius=r, patch_radius=f)
        assert out.tobytes() == u.tobytes()


@pytest.mark.gpu
def test_a_nan_pixel_stays_nan_and_does_not_spread(gpu_ctx):
    rng = np.random.default_rng(5)
    W, H, n = 48, 40, 16
    S, Q, _, _ = _plain_frame(rng, W, H, n)
    px, py = 20, 17
    tiles = [t for t in generate_tiles(W, H, (8, 8))]
    # the same frame with that pixel made invalid through its count: rects that leave it as its own 1x1 rect with n = 1
    split = []
    for (l, t, w, h) in tiles:
        if l <= px < l + w and t <= py < t + h:
            for y in range(t, t + h):
                for x in range(l, l + w):
                    if (x, y) != (px, py):
                        split.append(((x, y, 1, 1), n))
            split.append(((px, py, 1, 1), 1))
        else:
            split.append(((l, t, w, h), n))
    by_count = render.denoise_arrays(gpu_ctx, S, Q, [r for r, _ in split], [c for _, c in split])
    S_nan = S.copy()
    S_nan[py, px, 1] = np.nan
    by_nan = render.denoise_arrays(gpu_ctx, S_nan, Q, tiles, [n] * len(tiles))
    assert np.isnan(by_nan[py, px, 1])
    mask = np.ones((H, W), dtype=bool)
    mask[py, px] = False
    assert np.isfinite(by_nan[mask]).all()
    assert by_nan[mask].tobytes() == by_count[mask].tobytes()
    # the pixel mattered: without it the window around it comes out differently
    plain = render.denoise_arrays(gpu_ctx, S, Q, tiles, [n] * len(tiles))
    assert not np.array_equal(plain[py - 10 : py + 11, px - 10 : px + 11][mask[py - 10 : py + 11, px - 10 : px + 11]],
                              by_nan[py - 10 : py + 11, px - 10 : px + 11][mask[py - 10 : py + 11, px - 10 : px + 11]])


@pytest.mark.gpu
def test_one_rect_equals_tiles_at_the_same_count_and_repeats(gpu_ctx):
    rng = np.random.default_rng(6)
    W, H, n = 77, 53, 12
    S, Q, rect, count = _plain_frame(rng, W, H, n)
    one = render.denoise_arrays(gpu_ctx, S, Q, rect, count)
    tiles = generate_tiles(W, H, (32, 32))
    many = render.denoise_arrays(gpu_ctx, S, Q, tiles, [n] * len(tiles))
    again = render.denoise_arrays(gpu_ctx, S, Q, tiles, [n] * len(tiles))
    assert one.tobytes() == many.tobytes() == again.tobytes()
    assert np.isfinite(one).all()


@pytest.mark.gpu
def test_device_framebuffers_and_a_repeat_on_the_same_buffers(gpu_ctx):
    """render.denoise on device buffers; the output buffer written twice gives the same bits."""
    rng = np.random.default_rng(7)
    W, H, n = 33, 31, 5
    S, Q, rect, count = _plain_frame(rng, W, H, n)
    fbs = [render.Framebuffer(gpu_ctx, W, H) for _ in range(3)]
    try:
        fbs[0].upload(S)
        fbs[1].upload(Q)
        render.denoise(gpu_ctx, fbs[0], fbs[1], rect, count, fbs[2], radius=4, patch_radius=2)
        first = fbs[2].download()
        render.denoise(gpu_ctx, fbs[0], fbs[1], rect, count, fbs[2], radius=4, patch_radius=2)
        assert fbs[2].download().tobytes() == first.tobytes()
        assert fbs[0].download().tobytes() == S.tobytes() and fbs[1].download().tobytes() == Q.tobytes()  # the inputs are untouched
    finally:
        for fb in fbs:
            fb.close()
    _agree(first, denoise_ref.denoise(S, Q, np.full((H, W), n), radius=4, patch_radius=2))


# ---------------------------------------------------------------- quality on a real render
def render_moments(ctx, scene, W, H, spp, seed, bounces=5):
    """(S, Q) of a full-frame render of `spp` samples with the given seed."""
    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=bounces, seed=seed)
    ds = render.DeviceScene(ctx, scene)
    fb, fb_sq = render.Framebuffer(ctx, W, H), render.Framebuffer(ctx, W, H)
    try:
        render.render_tiles(ctx, ds, st.camera_settings, st, generate_tiles(W, H, (32, 32)), fb, 0, spp, framebuffer_sq=fb_sq)
        return fb.download(), fb_sq.download()
    finally:
        fb.close(), fb_sq.close(), ds.close()


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


@pytest.fixture(scope="module")
def spheres_references(gpu_ctx):
    W, H = 256, 144
    sc = scenes.reflective_spheres()
    ref_a = render_moments(gpu_ctx, sc, W, H, 2048, seed=0x1234567)
    ref_b = render_moments(gpu_ctx, sc, W, H, 2048, seed=0x7654321)
    return sc, W, H, ref_a, ref_b


@pytest.mark.gpu
def test_denoised_16spp_is_closer_to_the_converged_frame(gpu_ctx, spheres_references):
    sc, W, H, (S_ref, _), _ = spheres_references
    ref = S_ref / 2048.0
    S, Q = render_moments(gpu_ctx, sc, W, H, 16, seed=scenes.SEED)
    noisy = S / 16.0
    den = render.denoise_arrays(gpu_ctx, S, Q, [(0, 0, W, H)], [16])
    ratio = rmse(den, ref) / rmse(noisy, ref)
    print("denoise quality: ReflectiveSpheres 256x144 16 spp: RMSE %.5g -> %.5g, ratio %.4f" % (rmse(noisy, ref), rmse(den, ref), ratio))
    assert ratio <= 0.75, ratio


@pytest.mark.gpu
def test_denoising_a_converged_frame_does_not_blur_it(gpu_ctx, spheres_references):
    sc, W, H, (S_a, Q_a), (S_b, _) = spheres_references
    a, b = S_a / 2048.0, S_b / 2048.0
    den = render.denoise_arrays(gpu_ctx, S_a, Q_a, [(0, 0, W, H)], [2048])
    ratio = rmse(den, b) / rmse(a, b)
    print("denoise quality: ReflectiveSpheres 256x144 2048 spp against a second 2048 spp frame: ratio %.4f" % ratio)
    assert ratio <= 1.05, ratio


# ---------------------------------------------------------------- the host paths
def _median_tile_error(ctx, W, H, spp, bounces, floor):
    """The median rmd_tile_error of the 32x32 tiles after the first `spp` samples: as an adaptive threshold, about half of the tiles finish at the
    first check."""
    tiles = generate_tiles(W, H, (32, 32))
    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=bounces, seed=scenes.SEED)
    ds = render.DeviceScene(ctx, scenes.reflective_spheres())
    fb, fb_sq = render.Framebuffer(ctx, W, H), render.Framebuffer(ctx, W, H)
    try:
        render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fb, 0, spp, framebuffer_sq=fb_sq)
        return float(np.median(render.tile_error(ctx, fb, fb_sq, spp, floor, tiles)))
    finally:
        fb.close(), fb_sq.close(), ds.close()


def _finished_tiles(handle):
    """The TileFinished tiles await_() would take (after the leading TileProgressed snapshots), without consuming them."""
    handle.async_await()
    tiles = []
    for m in handle._messages:
        if m.kind != "TileFinished":
            break
        tiles.append(m.tile)
    return tiles


def _assemble(tiles, W, H):
    S, Q = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    rects, counts = [], []
    for t in tiles:
        S[t.top : t.top + t.height, t.left : t.left + t.width] = t.data
        Q[t.top : t.top + t.height, t.left : t.left + t.width] = t.data_sq
        rects.append((t.left, t.top, t.width, t.height))
        counts.append(t.sample_count)
    return S, Q, rects, counts


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["one_pass", "progressive", "adaptive", "two_workers"])
def test_render_tiled_denoise_equals_rmd_denoise_over_the_tiles(gpu_ctx, form):
    W, H, spp = 96, 64, 12
    sc = scenes.reflective_spheres()
    kw = dict(sample_count=spp, tile_size=(32, 32), bounce_limit=4, seed=scenes.SEED, denoise=True, denoise_radius=5, denoise_patch=2)
    if form in ("progressive", "two_workers"):
        kw["samples_per_iteration"] = 4
    if form == "adaptive":
        kw.update(samples_per_iteration=3, adaptive_threshold=_median_tile_error(gpu_ctx, W, H, 3, 4, 0.05), adaptive_floor=0.05)
    st = Settings(scenes.camera(W, H), **kw)
    handle = render.render_tiled(sc, st, devices=(0, 0) if form == "two_workers" else (0,))
    tiles = _finished_tiles(handle)
    assert len(tiles) == len(generate_tiles(W, H, (32, 32)))
    assert all(t.data_sq is not None and t.data_sq.shape == t.data.shape for t in tiles)
    S, Q, rects, counts = _assemble(tiles, W, H)
    if form == "adaptive":
        assert min(counts) < spp, "no tile finished early: the adaptive form was not exercised"
    else:  # the sums the tiles carry are those of one full-frame moments render
        S1, Q1 = render_moments(gpu_ctx, sc, W, H, spp, scenes.SEED, bounces=4)
        assert S.tobytes() == S1.tobytes() and Q.tobytes() == Q1.tobytes()
    expected = render.denoise_arrays(gpu_ctx, S, Q, rects, counts, radius=5, patch_radius=2, k=0.45, alpha=1.0)
    got = handle.await_()
    assert got.tobytes() == expected.tobytes()
    # denoise off: the same render gives the plain means
    st.denoise = False
    plain = render.render_tiled(sc, st, devices=(0,))
    plain.async_await()
    if form != "adaptive":
        with np.errstate(all="ignore"):
            assert plain.await_().tobytes() == (S / float(spp)).tobytes()


def _cli():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


@pytest.mark.gpu
@pytest.mark.parametrize("spi,gpus,extra", [(0, 1, []), (4, 1, []), (4, 2, []), (3, 1, ["--adaptive", "median", "--adaptive-floor", "0.05"]),
                                            (0, 1, ["--denoise-radius", "12", "--denoise-patch", "4", "--denoise-k", "0.8", "--denoise-alpha", "0.5"])])
def test_cli_denoise_equals_the_python_path(gpu_ctx, tmp_path, spi, gpus, extra):
    cli = _cli()
    W, H, spp, bounces = 96, 64, 12, 4
    if "median" in extra:  # an adaptive threshold that finishes about half of the tiles at the first check
        extra = [("%.17g" % _median_tile_error(gpu_ctx, W, H, spi, bounces, 0.05)) if e == "median" else e for e in extra]
    ppm, raw = tmp_path / "o.ppm", tmp_path / "o.f64"
    os.environ["RAYMOND_REHEARSE_ON_DEVICE0"] = "1"
    try:
        r = subprocess.run([cli, "render", "spheres", str(W), str(H), str(spp), str(bounces), str(ppm), "--raw", str(raw), "--spi", str(spi),
                            "--gpus", str(gpus), "--denoise", "1", *extra], capture_output=True, text=True)
    finally:
        os.environ.pop("RAYMOND_REHEARSE_ON_DEVICE0", None)
    assert r.returncode == 0, r.stderr
    img_cpp = np.fromfile(raw).reshape(H, W, 3)
    opts = dict(zip(extra[0::2], extra[1::2]))
    kw = dict(sample_count=spp, tile_size=(32, 32), bounce_limit=bounces, seed=scenes.SEED, samples_per_iteration=spi, denoise=True,
              denoise_radius=int(opts.get("--denoise-radius", 10)), denoise_patch=int(opts.get("--denoise-patch", 3)),
              denoise_k=float(opts.get("--denoise-k", 0.45)), denoise_alpha=float(opts.get("--denoise-alpha", 1.0)))
    if "--adaptive" in opts:
        kw.update(adaptive_threshold=float(opts["--adaptive"]), adaptive_floor=float(opts["--adaptive-floor"]))
    handle = render.render_tiled(scenes.reflective_spheres(), Settings(scenes.camera(W, H), **kw), devices=(0,) * gpus)
    handle.async_await()
    img_py = handle.await_()
    assert np.isfinite(img_py).all()
    assert img_cpp.tobytes() == img_py.tobytes()
