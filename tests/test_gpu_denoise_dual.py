"""rmd_denoise_dual and rmd_tile_error_dual on the device: the kernels against the numpy restatement (tests/denoise_dual_ref.py), the exact
properties of the definition, the host paths (Python render_tiled / await_, the C++ mirror through raymond_cli), and what the error estimate
is for: adaptive sampling that beats uniform sampling at the same cost, and a per-tile estimate that ranks the tiles as their true error does.

The frames, counts, poison and tolerance are test_gpu_denoise.py's own (imported from it)."""
import math
import os
import subprocess

import numpy as np
import pytest

import denoise_dual_ref
import denoise_ref
from raymond_amd import render, scenes
from raymond_amd.scene import Settings, generate_tiles
from test_gpu_denoise import CASES, _agree, _finished_tiles, _moments, _poison, _tiles_with_counts, render_moments, rmse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")


def _device(ctx, S_a, Q_a, S_b, Q_b, rects, counts_a, counts_b, tiles=None, **params):
    """rmd_denoise_dual on uploaded halves, then rmd_tile_error_dual over `tiles` (default: the rects) -> (out, err, tile errors)."""
    H, W = S_a.shape[:2]
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(5)]
    err = render.ErrorImage(ctx, W, H)
    try:
        for fb, arr in zip(fbs, (S_a, Q_a, S_b, Q_b)):
            fb.upload(arr)
        render.denoise_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), rects, counts_a, counts_b, fbs[4], err, **params)
        return fbs[4].download(), err.download(), render.tile_error_dual(ctx, err, rects if tiles is None else tiles)
    finally:
        for fb in fbs + [err]:
            fb.close()


def _two_halves(rng, W, H, tw=8, th=16, poison=True):
    """Two halves over one tiling with unequal per-rect counts (each with a 1 and a 0 somewhere), one tile uncovered, poisoned sums."""
    rects, counts_a = _tiles_with_counts(W, H, tw, th, rng) if W * H > 1 else ([(0, 0, 1, 1)], [9])
    counts_b = [int(c) for c in rng.integers(2, 65, len(rects))] if W * H > 1 else [5]
    if len(rects) >= 6:
        counts_b[4], counts_b[5] = 0, 1
    n_a, n_b = denoise_ref.count_image(W, H, rects, counts_a), denoise_ref.count_image(W, H, rects, counts_b)
    S_a, Q_a = _moments(rng, n_a)
    S_b, Q_b = _moments(rng, n_b)
    if poison and W * H > 1:
        _poison(S_a, Q_a, rng)
        _poison(S_b, Q_b, rng)
    return (S_a, Q_a, S_b, Q_b), rects, counts_a, counts_b, n_a, n_b


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1, 1), (5, 200), (37, 23), (64, 48)])
def test_kernel_matches_the_restatement(gpu_ctx, W, H):
    rng = np.random.default_rng(W * 1000 + H + 7)
    halves, rects, counts_a, counts_b, n_a, n_b = _two_halves(rng, W, H)
    tiles = rects + [(0, 0, W, H), (W - 1, H - 1, 1, 1), (0, 0, 0, 0)]
    for r, f, k, alpha in CASES:
        out, err, terr = _device(gpu_ctx, *halves, rects, counts_a, counts_b, tiles=tiles, radius=r, patch_radius=f, k=k, alpha=alpha)
        out_ref, err_ref = denoise_dual_ref.denoise_dual(*halves, n_a, n_b, radius=r, patch_radius=f, k=k, alpha=alpha)
        _agree(out, out_ref)
        _agree(err, err_ref)
        _agree(terr, denoise_dual_ref.tile_error_dual(err_ref, tiles))
        assert terr[-1] == 0.0  # a rect without pixels


@pytest.mark.gpu
def test_radius_zero_is_the_closed_form_bit_for_bit(gpu_ctx):
    rng = np.random.default_rng(3)
    W, H = 45, 29
    halves, rects, counts_a, counts_b, n_a, n_b = _two_halves(rng, W, H, 16, 8)
    halves[0][3, 3] = -0.0
    for f in (0, 1, 4):
        out, err, _ = _device(gpu_ctx, *halves, rects, counts_a, counts_b, radius=0, patch_radius=f)
        out_ref, err_ref = denoise_dual_ref.denoise_dual(*halves, n_a, n_b, radius=0, patch_radius=f)  # (held to the closed form on the CPU)
        assert out.tobytes() == out_ref.tobytes()
        assert err.tobytes() == err_ref.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 12])
def test_equal_halves_give_the_device_rmd_denoise_and_no_error(gpu_ctx, n):
    """A == B: err == 0 exactly; out is rmd_denoise of that half bit for bit at a power-of-two count, and within the one rounding of n * f that the
    stated operation order leaves at any other (raymond_hip.h)."""
    rng = np.random.default_rng(4)
    W, H = 70, 41
    rects = generate_tiles(W, H, (32, 16))
    counts = [n] * len(rects)
    counts[2] = 1  # a tile that is not valid
    n_img = denoise_ref.count_image(W, H, rects, counts)
    S, Q = _moments(rng, n_img)
    _poison(S, Q, rng)
    for r, f in ((1, 0), (4, 2), (10, 3), (12, 4)):
        out, err, terr = _device(gpu_ctx, S, Q, S, Q, rects, counts, counts, radius=r, patch_radius=f)
        single = render.denoise_arrays(gpu_ctx, S, Q, rects, counts, radius=r, patch_radius=f)
        _, _, valid = denoise_ref.mean_and_variance(S, Q, n_img)
        assert np.all(err[valid] == 0.0) and np.isnan(err[~valid]).all()
        if n == 8:
            assert out[valid].tobytes() == single[valid].tobytes()
        else:
            assert np.all(np.abs(out[valid] - single[valid]) <= np.spacing(np.abs(single[valid])))
        with np.errstate(all="ignore"):
            merged = (S + S) / (n_img + n_img).astype(np.float64)[..., None]
        assert out[~valid].tobytes() == merged[~valid].tobytes()
        assert terr[2] == np.inf and all(t == 0.0 or t == np.inf for t in terr)


@pytest.mark.gpu
def test_one_rect_equals_tiles_at_the_same_counts_and_a_repeat_gives_the_same_bytes(gpu_ctx):
    rng = np.random.default_rng(6)
    W, H, na, nb = 77, 53, 12, 7
    n_a, n_b = np.full((H, W), na), np.full((H, W), nb)
    halves = _moments(rng, n_a) + _moments(rng, n_b)
    tiles = generate_tiles(W, H, (32, 32))
    one = _device(gpu_ctx, *halves, [(0, 0, W, H)], [na], [nb], tiles=tiles)
    many = _device(gpu_ctx, *halves, tiles, [na] * len(tiles), [nb] * len(tiles))
    assert one[0].tobytes() == many[0].tobytes() and one[1].tobytes() == many[1].tobytes() and one[2].tobytes() == many[2].tobytes()
    assert np.isfinite(one[0]).all() and np.isfinite(one[1]).all() and (one[1] > 0.0).any()
    # the same buffers twice; without an error image the frame is the same
    fbs = [render.Framebuffer(gpu_ctx, W, H) for _ in range(5)]
    err = render.ErrorImage(gpu_ctx, W, H)
    try:
        for fb, arr in zip(fbs, halves):
            fb.upload(arr)
        frames = []
        for e in (err, err, None):
            render.denoise_dual(gpu_ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), tiles, [na] * len(tiles), [nb] * len(tiles), fbs[4], e)
            frames.append((fbs[4].download().tobytes(), err.download().tobytes()))
        assert frames[0] == frames[1] == frames[2] == (many[0].tobytes(), many[1].tobytes())
        assert all(fb.download().tobytes() == arr.tobytes() for fb, arr in zip(fbs, halves))  # the inputs are untouched
    finally:
        for fb in fbs + [err]:
            fb.close()


# ---------------------------------------------------------------- the host paths
def _assemble_dual(tiles, W, H):
    halves = [np.zeros((H, W, 3)) for _ in range(4)]
    rects, counts_a, counts_b = [], [], []
    for t in tiles:
        for dst, src in zip(halves, (t.data_a, t.data_sq_a, t.data_b, t.data_sq_b)):
            dst[t.top : t.top + t.height, t.left : t.left + t.width] = src
        rects.append((t.left, t.top, t.width, t.height))
        counts_a.append(t.count_a)
        counts_b.append(t.count_b)
    return halves, rects, counts_a, counts_b


def _dual_settings(W, H, spp, spi, bounces, **kw):
    return Settings(scenes.camera(W, H), sample_count=spp, tile_size=(32, 32), bounce_limit=bounces, seed=scenes.SEED, samples_per_iteration=spi, denoise=True,
                    denoise_dual=True, **kw)


def _median_dual_tile_error(ctx, W, H, spp, spi, bounces, **params):
    """The median rmd_tile_error_dual of the 32x32 tiles of a uniform dual render of `spp` samples: as a threshold, about half of the tiles finish
    at the first check (as _median_tile_error for the raw rule)."""
    handle = render.render_tiled(scenes.reflective_spheres(), _dual_settings(W, H, spp, spi, bounces), devices=(0,))
    halves, rects, counts_a, counts_b = _assemble_dual(_finished_tiles(handle), W, H)
    return float(np.median(_device(ctx, *halves, rects, counts_a, counts_b, **params)[2]))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["progressive", "odd_passes", "adaptive"])
def test_render_tiled_dual_equals_rmd_denoise_dual_over_the_tiles(gpu_ctx, form):
    W, H, bounces = 96, 64, 4
    spp, spi = (12, 3) if form != "odd_passes" else (10, 4)  # odd_passes: passes of 4, 4 and 2 samples -> 6 in A, 4 in B
    sc = scenes.reflective_spheres()
    params = dict(radius=5, patch_radius=2, k=0.45, alpha=1.0)
    kw = dict(denoise_radius=5, denoise_patch=2)
    if form == "adaptive":
        kw.update(adaptive_denoised_threshold=_median_dual_tile_error(gpu_ctx, W, H, 6, 3, bounces, **params), adaptive_min_samples=6)
    handle = render.render_tiled(sc, _dual_settings(W, H, spp, spi, bounces, **kw), devices=(0,))
    tiles = _finished_tiles(handle)
    assert len(tiles) == len(generate_tiles(W, H, (32, 32)))
    halves, rects, counts_a, counts_b = _assemble_dual(tiles, W, H)
    for t in tiles:
        assert t.sample_count == t.count_a + t.count_b
        assert t.data.tobytes() == (t.data_a + t.data_b).tobytes() and t.data_sq.tobytes() == (t.data_sq_a + t.data_sq_b).tobytes()
    if form == "adaptive":
        early = [t for t in tiles if t.sample_count < spp]
        assert early and len(early) < len(tiles), "the adaptive form was not exercised"
        assert all(t.count_a == t.count_b and t.error is not None and t.error <= handle.settings.adaptive_denoised_threshold for t in early)
    else:
        assert set(zip(counts_a, counts_b)) == ({(6, 6)} if form == "progressive" else {(6, 4)})
        # the halves are the moments renders of their own sample ranges: pass j covers samples [j * spi, (j + 1) * spi) and goes to A when j is even
        st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=bounces, seed=scenes.SEED)
        ds = render.DeviceScene(gpu_ctx, sc)
        fbs = [render.Framebuffer(gpu_ctx, W, H) for _ in range(4)]
        try:
            for j, begin in enumerate(range(0, spp, spi)):
                render.render_tiles(gpu_ctx, ds, st.camera_settings, st, generate_tiles(W, H, (32, 32)), fbs[2 * (j & 1)], begin, min(spi, spp - begin),
                                    framebuffer_sq=fbs[2 * (j & 1) + 1])
            assert all(fb.download().tobytes() == h.tobytes() for fb, h in zip(fbs, halves))
        finally:
            for o in fbs + [ds]:
                o.close()
    expected, _, _ = _device(gpu_ctx, *halves, rects, counts_a, counts_b, **params)
    got = handle.await_()
    assert got.tobytes() == expected.tobytes()


@pytest.mark.gpu
def test_with_the_new_settings_off_the_renders_are_the_plain_and_denoised_ones(gpu_ctx):
    """denoise_dual False and adaptive_denoised_threshold 0, given explicitly: the message stream (kinds, rects, counts, sums) and the awaited
    frames are those of the renders without the two settings — progress snapshots at every pass from one buffer, then the finished tiles."""
    W, H, spp, spi, bounces = 96, 64, 8, 4, 4
    sc = scenes.reflective_spheres()
    tiles = generate_tiles(W, H, (32, 32))
    S4, _ = render_moments(gpu_ctx, sc, W, H, 4, scenes.SEED, bounces=bounces)
    S8, Q8 = render_moments(gpu_ctx, sc, W, H, 8, scenes.SEED, bounces=bounces)
    for denoise in (False, True):
        st = Settings(scenes.camera(W, H), sample_count=spp, tile_size=(32, 32), bounce_limit=bounces, seed=scenes.SEED, samples_per_iteration=spi,
                      denoise=denoise, denoise_dual=False, adaptive_denoised_threshold=0.0, adaptive_min_samples=0)
        handle = render.render_tiled(sc, st, devices=(0,))
        msgs = list(handle._messages)
        assert [m.kind for m in msgs] == ["TileProgressed"] * len(tiles) + ["TileFinished"] * len(tiles)
        for m, rect in zip(msgs, tiles + tiles):
            t = m.tile
            l, tp, w, h = rect
            assert (t.left, t.top, t.width, t.height) == rect
            src, n = (S4, 4) if m.kind == "TileProgressed" else (S8, 8)
            assert t.sample_count == n and t.data.tobytes() == src[tp : tp + h, l : l + w].tobytes()
            assert t.data_a is None and t.data_b is None and t.count_a is None and t.error is None
            assert (t.data_sq is not None) == (denoise and m.kind == "TileFinished")
            if t.data_sq is not None:
                assert t.data_sq.tobytes() == Q8[tp : tp + h, l : l + w].tobytes()
        handle.async_await()
        got = handle.await_()
        expected = render.denoise_arrays(gpu_ctx, S8, Q8, tiles, [8] * len(tiles)) if denoise else S8 / 8.0
        assert got.tobytes() == expected.tobytes()


def _cli():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


@pytest.mark.gpu
@pytest.mark.parametrize("spp,spi,extra", [(12, 3, []), (10, 4, ["--denoise-radius", "12", "--denoise-patch", "4", "--denoise-k", "0.8", "--denoise-alpha", "0.5"]),
                                           (12, 3, ["--adaptive-denoised", "median", "--adaptive-min", "6"])])
def test_cli_denoise_dual_equals_the_python_path(gpu_ctx, tmp_path, spp, spi, extra):
    cli = _cli()
    W, H, bounces = 96, 64, 4
    if "median" in extra:  # a threshold that finishes about half of the tiles at the first check
        extra = [("%.17g" % _median_dual_tile_error(gpu_ctx, W, H, 6, spi, bounces)) if e == "median" else e for e in extra]
    ppm, raw = tmp_path / "o.ppm", tmp_path / "o.f64"
    r = subprocess.run([cli, "render", "spheres", str(W), str(H), str(spp), str(bounces), str(ppm), "--raw", str(raw), "--spi", str(spi), "--denoise", "1",
                        "--denoise-dual", "1", *extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img_cpp = np.fromfile(raw).reshape(H, W, 3)
    opts = dict(zip(extra[0::2], extra[1::2]))
    kw = dict(denoise_radius=int(opts.get("--denoise-radius", 10)), denoise_patch=int(opts.get("--denoise-patch", 3)),
              denoise_k=float(opts.get("--denoise-k", 0.45)), denoise_alpha=float(opts.get("--denoise-alpha", 1.0)))
    if "--adaptive-denoised" in opts:
        kw.update(adaptive_denoised_threshold=float(opts["--adaptive-denoised"]), adaptive_min_samples=int(opts["--adaptive-min"]))
    handle = render.render_tiled(scenes.reflective_spheres(), _dual_settings(W, H, spp, spi, bounces, **kw), devices=(0,))
    if "--adaptive-denoised" in opts:
        counts = [t.sample_count for t in _finished_tiles(handle)]
        assert min(counts) < spp and max(counts) == spp, "the adaptive form was not exercised"
    handle.async_await()
    img_py = handle.await_()
    assert np.isfinite(img_py).all()
    assert img_cpp.tobytes() == img_py.tobytes()


# ---------------------------------------------------------------- what the estimate is for
QW, QH, QBOUNCES = 256, 144, 5


@pytest.fixture(scope="module")
def converged(gpu_ctx):
    """The 2,048 spp frame of seed + 1: what every error below is measured against (its own noise is part of every RMSE)."""
    S, _ = render_moments(gpu_ctx, scenes.reflective_spheres(), QW, QH, 2048, seed=scenes.SEED + 1, bounces=QBOUNCES)
    return S / 2048.0


def _tile_rms(img, ref, tiles):
    return np.array([math.sqrt(np.mean((img[t : t + h, l : l + w] - ref[t : t + h, l : l + w]) ** 2)) for (l, t, w, h) in tiles])


def _ranks(x):
    """Ranks 1 .. n, ties sharing the mean of their ranks."""
    x = np.asarray(x, dtype=np.float64)
    order = np.argsort(x, kind="stable")
    ranks = np.empty(len(x))
    i = 0
    while i < len(x):
        j = i
        while j + 1 < len(x) and x[order[j + 1]] == x[order[i]]:
            j += 1
        ranks[order[i : j + 1]] = (i + j) / 2.0 + 1.0
        i = j + 1
    return ranks


def _spearman(a, b):
    return float(np.corrcoef(_ranks(a), _ranks(b))[0, 1])


@pytest.mark.gpu
def test_adaptive_sampling_by_the_filtered_error_beats_uniform_sampling(gpu_ctx, converged):
    """ReflectiveSpheres 256x144, 5 bounces, seed scenes.SEED, 32x32 tiles, passes of 8, at most 128 samples, no check below 32, threshold = the
    median rmd_tile_error_dual of a uniform 32 spp dual render.  The awaited frame's RMSE against the 2,048 spp frame of seed + 1 must not
    exceed that of uniform sampling at the adaptive run's mean spp rounded UP to a multiple of 16, filtered by rmd_denoise and by
    rmd_denoise_dual: the bar is 1.0 against frames of the existing paths.  (A CPU prototype of this configuration gave 0.01491 at 62.0 spp
    against 0.01659 and 0.01577 at 64.)"""
    sc = scenes.reflective_spheres()
    tiles = generate_tiles(QW, QH, (32, 32))
    threshold = _median_dual_tile_error(gpu_ctx, QW, QH, 32, 8, QBOUNCES)
    handle = render.render_tiled(sc, _dual_settings(QW, QH, 128, 8, QBOUNCES, adaptive_denoised_threshold=threshold, adaptive_min_samples=32), devices=(0,))
    finished = _finished_tiles(handle)
    assert len(finished) == len(tiles)
    counts = [t.sample_count for t in finished]
    mean_spp = sum(t.sample_count * t.width * t.height for t in finished) / float(QW * QH)
    adaptive = handle.await_()
    uniform_spp = int(math.ceil(mean_spp / 16.0)) * 16
    S, Q = render_moments(gpu_ctx, sc, QW, QH, uniform_spp, seed=scenes.SEED, bounces=QBOUNCES)
    uniform_single = render.denoise_arrays(gpu_ctx, S, Q, [(0, 0, QW, QH)], [uniform_spp])
    uniform_dual = render.render_tiled(sc, _dual_settings(QW, QH, uniform_spp, 8, QBOUNCES), devices=(0,))
    uniform_dual.async_await()
    uniform_dual = uniform_dual.await_()
    e_adaptive, e_single, e_dual = rmse(adaptive, converged), rmse(uniform_single, converged), rmse(uniform_dual, converged)
    print("dual adaptive quality: threshold %.6g, mean spp %.2f (min %d, max %d, %d of %d tiles early): RMSE %.5f; uniform %d spp: rmd_denoise %.5f, "
          "rmd_denoise_dual %.5f; ratios %.4f, %.4f" % (threshold, mean_spp, min(counts), max(counts), sum(c < 128 for c in counts), len(counts), e_adaptive,
                                                       uniform_spp, e_single, e_dual, e_adaptive / e_single, e_adaptive / e_dual))
    assert min(counts) < 128, "no tile finished early"
    assert max(counts) == 128, "no tile reached the sample count"
    assert e_adaptive <= e_single, (e_adaptive, e_single)
    assert e_adaptive <= e_dual, (e_adaptive, e_dual)


@pytest.mark.gpu
def test_the_tile_error_ranks_the_tiles_as_their_true_error_does(gpu_ctx, converged):
    """Spearman's rank correlation, over the 32x32 tiles at uniform 32 spp, of rmd_tile_error_dual with the per-tile RMS error of the delivered
    frame against the 2,048 spp frame.  The device's value lies within 0.01 of the numpy restatement's on the same sums (the device's exp may move
    a near-tie), and the restatement's exceeds the same correlation for today's rule: rmd_tile_error against the rmd_denoise frame's per-tile
    error.  (CPU prototype: 0.88 against 0.02.)"""
    sc = scenes.reflective_spheres()
    tiles = generate_tiles(QW, QH, (32, 32))
    handle = render.render_tiled(sc, _dual_settings(QW, QH, 32, 8, QBOUNCES), devices=(0,))
    halves, rects, counts_a, counts_b = _assemble_dual(_finished_tiles(handle), QW, QH)
    assert set(counts_a) == set(counts_b) == {16}
    out, err, terr = _device(gpu_ctx, *halves, rects, counts_a, counts_b, tiles=tiles)
    rho_dev = _spearman(terr, _tile_rms(out, converged, tiles))
    n16 = np.full((QH, QW), 16)
    out_ref, err_ref = denoise_dual_ref.denoise_dual(*halves, n16, n16)
    terr_ref = denoise_dual_ref.tile_error_dual(err_ref, tiles)
    true_ref = _tile_rms(out_ref, converged, tiles)
    rho_ref = _spearman(terr_ref, true_ref)
    # today's rule on the same 32 samples
    S, Q = render_moments(gpu_ctx, sc, QW, QH, 32, seed=scenes.SEED, bounces=QBOUNCES)
    fb, fb_sq = render.Framebuffer(gpu_ctx, QW, QH), render.Framebuffer(gpu_ctx, QW, QH)
    try:
        fb.upload(S), fb_sq.upload(Q)
        raw_rule = render.tile_error(gpu_ctx, fb, fb_sq, 32, 1e-3, tiles)
    finally:
        fb.close(), fb_sq.close()
    single = render.denoise_arrays(gpu_ctx, S, Q, [(0, 0, QW, QH)], [32])
    rho_raw = _spearman(raw_rule, _tile_rms(single, converged, tiles))
    ratio = np.median(terr_ref / true_ref)
    print("dual rank correlation at 32 spp: device %.4f, restatement %.4f, rmd_tile_error against rmd_denoise %.4f; median estimate / true error %.3f"
          % (rho_dev, rho_ref, rho_raw, ratio))
    assert abs(rho_dev - rho_ref) <= 0.01, (rho_dev, rho_ref)
    assert rho_ref > rho_raw, (rho_ref, rho_raw)
