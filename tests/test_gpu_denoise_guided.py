"""rmd_denoise_guided on the device: the kernel against the numpy restatement (tests/denoise_guided_ref.py), its exact properties, the host
paths that use it (Python render_tiled / await_, the C++ mirror through raymond_cli), and its quality on real renders against rmd_denoise."""
import os
import subprocess

import numpy as np
import pytest

import denoise_guided_ref as gref
import denoise_ref
import test_gpu_denoise as tgd
from raymond_amd import render, scenes
from raymond_amd.scene import Settings, generate_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _features(rng, n_img):
    """Feature sums and sums of squares of n samples per pixel: normals and albedos with steps, a depth ramp with a step, noise on all of them
    whose level varies, some pixels that are misses, and NaN / inf poison."""
    H, W = n_img.shape
    y, x = np.mgrid[0:H, 0:W]
    f = np.zeros((H, W, 7))
    f[..., 0] = np.where(x % 11 < 5, 0.0, 0.6)
    f[..., 1] = np.where(y % 7 < 3, 0.8, 0.0)
    f[..., 2] = 1.0 - 0.5 * ((x + y) % 2)
    f[..., 3:6] = np.stack([np.where(x < W // 2, 0.8, 0.2), 0.2 + 0.0 * x, np.where(y < H // 2, 0.2, 0.8)], axis=-1)
    f[..., 6] = 3.0 + 0.01 * x + np.where(x % 13 < 6, 0.0, 0.5)
    f[(x + 2 * y) % 17 == 0] = 0.0  # misses
    n = np.maximum(n_img, 0).astype(np.float64)[..., None]
    sigma = rng.uniform(0.0, 0.05, (H, W, 1)) * (x % 5 == 0)[..., None]
    mean = f + rng.normal(0.0, 1.0, (H, W, 7)) * sigma
    F = mean * n
    G = F * mean + rng.uniform(0.0, 1.0, (H, W, 7)) * sigma * sigma * np.maximum(n - 1.0, 0.0)
    for value, arr in ((np.nan, F), (np.inf, F), (np.inf, G), (np.nan, G)):
        for _ in range(max(1, H * W // 300)):
            arr[rng.integers(0, H), rng.integers(0, W), rng.integers(0, 7)] = value
    return F, G


@pytest.mark.parametrize("W,H", [(1, 1), (5, 200), (37, 23), (64, 48)])
def test_guided_kernel_matches_the_restatement(gpu_ctx, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    rects, counts = tgd._tiles_with_counts(W, H, 8, 16, rng) if W * H > 1 else ([(0, 0, 1, 1)], [9])
    n_img = denoise_ref.count_image(W, H, rects, counts)
    S, Q = tgd._moments(rng, n_img)
    F, G = _features(rng, n_img)
    if W * H > 1:
        tgd._poison(S, Q, rng)
    for i, (r, f, k, alpha) in enumerate(tgd.CASES):
        k_f, tau = ((0.6, 1e-3), (0.3, 1e-2), (1.5, 1e-4))[i % 3]
        dev = render.denoise_guided_arrays(gpu_ctx, S, Q, F, G, rects, counts, radius=r, patch_radius=f, k=k, alpha=alpha, k_f=k_f, tau=tau)
        ref = gref.denoise_guided(S, Q, F, G, n_img, radius=r, patch_radius=f, k=k, alpha=alpha, k_f=k_f, tau=tau)
        tgd._agree(dev, ref)
        if r >= 3 and W * H > 100:  # the features mattered
            assert not np.array_equal(ref, denoise_ref.denoise(S, Q, n_img, radius=r, patch_radius=f, k=k, alpha=alpha), equal_nan=True)


@pytest.mark.parametrize("r,f", [(3, 1), (10, 3), (12, 4)])
def test_zero_and_null_features_are_rmd_denoise_bit_for_bit(gpu_ctx, r, f):
    rng = np.random.default_rng(11)
    W, H = 70, 41
    rects, counts = tgd._tiles_with_counts(W, H, 16, 8, rng)
    n_img = denoise_ref.count_image(W, H, rects, counts)
    S, Q = tgd._moments(rng, n_img)
    tgd._poison(S, Q, rng)
    plain = render.denoise_arrays(gpu_ctx, S, Q, rects, counts, radius=r, patch_radius=f)
    Z = np.zeros((H, W, 7))
    zero = render.denoise_guided_arrays(gpu_ctx, S, Q, Z, Z, rects, counts, radius=r, patch_radius=f)
    null = render.denoise_guided_arrays(gpu_ctx, S, Q, None, None, rects, counts, radius=r, patch_radius=f, k_f=float("nan"), tau=-1.0)
    assert plain.tobytes() == zero.tobytes() == null.tobytes()
    assert np.isfinite(plain).any()


@pytest.mark.parametrize("seed", [1, 2])
def test_step_edge_on_the_device(gpu_ctx, seed):
    S, Q, F, G, n, truth = gref.step_edge_frame(seed)
    H, W = n.shape
    rect, count = [(0, 0, W, H)], [int(n[0, 0])]
    un = render.denoise_arrays(gpu_ctx, S, Q, rect, count, radius=10, patch_radius=3, k=0.45, alpha=1.0)
    gd = render.denoise_guided_arrays(gpu_ctx, S, Q, F, G, rect, count, radius=10, patch_radius=3, k=0.45, alpha=1.0, k_f=0.6, tau=1e-3)
    ru, rg = gref.band_rmse(un, truth), gref.band_rmse(gd, truth)
    print("step edge on the device, seed %d: band RMSE unguided %.4f guided %.4f ratio %.3f" % (seed, ru, rg, rg / ru))
    assert rg <= 0.6 * ru


def test_hit_miss_frame_on_the_device_is_exact(gpu_ctx):
    S, Q, F, G, n, u = gref.hit_miss_frame()
    H, W = n.shape
    rect, count = [(0, 0, W, H)], [int(n[0, 0])]
    un = render.denoise_arrays(gpu_ctx, S, Q, rect, count)
    gd = render.denoise_guided_arrays(gpu_ctx, S, Q, F, G, rect, count)
    assert gd.tobytes() == u.tobytes()
    assert np.abs(un - u).max() > 0.2
    F2 = F.copy()
    F2[12, 24, 1] = np.nan
    g2 = render.denoise_guided_arrays(gpu_ctx, S, Q, F2, G, rect, count)
    assert g2[12, 24].tobytes() == un[12, 24].tobytes() and np.isfinite(g2).all()
    mean = render.denoise_guided_arrays(gpu_ctx, S, Q, F2, G, rect, count, radius=0)
    assert mean.tobytes() == u.tobytes()  # radius 0: S / n


# ---------------------------------------------------------------- the host paths
def _direct_features(ctx, sc, st, rects, counts):
    """One rmd_render_features call per rect at its own count, into fresh buffers: what await_() has to have rendered."""
    cam = st.camera_settings
    W, H = cam.backbuffer_width, cam.backbuffer_height
    ds = render.DeviceScene(ctx, sc)
    fb, fb_sq = render.FeatureBuffer(ctx, W, H), render.FeatureBuffer(ctx, W, H)
    try:
        for r, c in zip(rects, counts):
            render.render_features(ctx, ds, cam, st, [r], fb, 0, c, features_sq=fb_sq)
        return fb.download(), fb_sq.download()
    finally:
        fb.close(), fb_sq.close(), ds.close()


@pytest.mark.parametrize("form", ["one_pass", "progressive", "adaptive", "two_workers"])
def test_render_tiled_with_features_equals_the_direct_calls(gpu_ctx, form):
    W, H, spp = 96, 64, 12
    sc = scenes.reflective_spheres()
    kw = dict(sample_count=spp, tile_size=(32, 32), bounce_limit=4, seed=scenes.SEED, denoise=True, denoise_radius=5, denoise_patch=2,
              denoise_features=True, denoise_feature_k=0.8, denoise_feature_tau=2e-3)
    if form in ("progressive", "two_workers"):
        kw["samples_per_iteration"] = 4
    if form == "adaptive":
        kw.update(samples_per_iteration=3, adaptive_threshold=tgd._median_tile_error(gpu_ctx, W, H, 3, 4, 0.05), adaptive_floor=0.05)
    st = Settings(scenes.camera(W, H), **kw)
    handle = render.render_tiled(sc, st, devices=(0, 0) if form == "two_workers" else (0,))
    tiles = tgd._finished_tiles(handle)
    S, Q, rects, counts = tgd._assemble(tiles, W, H)
    if form == "adaptive":
        assert min(counts) < spp, "no tile finished early: the adaptive form was not exercised"
    F, G = _direct_features(gpu_ctx, sc, st, rects, counts)
    assert F.any()
    expected = render.denoise_guided_arrays(gpu_ctx, S, Q, F, G, rects, counts, radius=5, patch_radius=2, k=0.45, alpha=1.0, k_f=0.8, tau=2e-3)
    got = handle.await_()
    assert got.tobytes() == expected.tobytes()
    unguided = render.denoise_arrays(gpu_ctx, S, Q, rects, counts, radius=5, patch_radius=2)
    assert got.tobytes() != unguided.tobytes()
    # denoise_features off: the same render gives rmd_denoise's frame
    st.denoise_features = False
    plain = render.render_tiled(sc, st, devices=(0,))
    plain.async_await()
    if form != "adaptive":
        assert plain.await_().tobytes() == unguided.tobytes()


def _cli():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return tgd.CLI


@pytest.mark.parametrize("spi,gpus,extra", [(0, 1, []), (4, 2, []), (3, 1, ["--adaptive", "median", "--adaptive-floor", "0.05"]),
                                            (0, 1, ["--denoise-feature-k", "1.1", "--denoise-feature-tau", "0.004", "--aperture", "0.05"])])
def test_cli_with_features_equals_the_python_path(gpu_ctx, tmp_path, spi, gpus, extra):
    cli = _cli()
    W, H, spp, bounces = 96, 64, 12, 4
    if "median" in extra:
        extra = [("%.17g" % tgd._median_tile_error(gpu_ctx, W, H, spi, bounces, 0.05)) if e == "median" else e for e in extra]
    ppm, raw, aov = tmp_path / "o.ppm", tmp_path / "o.f64", tmp_path / "aov.f64"
    os.environ["RAYMOND_REHEARSE_ON_DEVICE0"] = "1"
    try:
        r = subprocess.run([cli, "render", "spheres", str(W), str(H), str(spp), str(bounces), str(ppm), "--raw", str(raw), "--spi", str(spi),
                            "--gpus", str(gpus), "--denoise", "1", "--denoise-features", "1", "--dump-features", str(aov), *extra],
                           capture_output=True, text=True)
    finally:
        os.environ.pop("RAYMOND_REHEARSE_ON_DEVICE0", None)
    assert r.returncode == 0, r.stderr
    img_cpp = np.fromfile(raw).reshape(H, W, 3)
    opts = dict(zip(extra[0::2], extra[1::2]))
    ap = float(opts.get("--aperture", 0.0))
    kw = dict(sample_count=spp, tile_size=(32, 32), bounce_limit=bounces, seed=scenes.SEED, samples_per_iteration=spi, denoise=True,
              denoise_features=True, use_dof=ap > 0.0)
    if "--denoise-feature-k" in opts:
        kw.update(denoise_feature_k=float(opts["--denoise-feature-k"]), denoise_feature_tau=float(opts["--denoise-feature-tau"]))
    if "--adaptive" in opts:
        kw.update(adaptive_threshold=float(opts["--adaptive"]), adaptive_floor=float(opts["--adaptive-floor"]))
    st = Settings(scenes.camera(W, H, aperture_radius=ap), **kw)
    sc = scenes.reflective_spheres()
    handle = render.render_tiled(sc, st, devices=(0,) * gpus)
    tiles = tgd._finished_tiles(handle)
    _, _, rects, counts = tgd._assemble(tiles, W, H)
    img_py = handle.await_()
    assert np.isfinite(img_py).all()
    assert img_cpp.tobytes() == img_py.tobytes()
    # --dump-features: the means, render_features / n
    F, _ = _direct_features(gpu_ctx, sc, st, rects, counts)
    n_img = denoise_ref.count_image(W, H, rects, counts).astype(np.float64)[..., None]
    assert np.fromfile(aov).reshape(H, W, 7).tobytes() == (F / n_img).tobytes()


# ---------------------------------------------------------------- quality on real renders
def _feature_sums(ctx, sc, W, H, spp, seed):
    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=seed)
    return _direct_features(ctx, sc, st, [(0, 0, W, H)], [spp])


@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_guided_at_its_defaults_is_no_worse_than_rmd_denoise_at_its_defaults(gpu_ctx, which):
    """256 x 144, 16 spp against 2,048 spp of another seed, RMSE in linear radiance; the comparator is rmd_denoise at its defaults on the same
    sums.  The converged-frame check of rmd_denoise (<= x1.05 against a second 2,048 spp frame) holds for the guided filter too."""
    W, H = 256, 144
    sc = scenes.reflective_spheres() if which == "spheres" else scenes.gold_dragon_standin(n=24)
    S_a, Q_a = tgd.render_moments(gpu_ctx, sc, W, H, 2048, seed=0x1234567)
    S_b, _ = tgd.render_moments(gpu_ctx, sc, W, H, 2048, seed=0x7654321)
    ref, ref_b = S_a / 2048.0, S_b / 2048.0
    S, Q = tgd.render_moments(gpu_ctx, sc, W, H, 16, seed=scenes.SEED)
    F, G = _feature_sums(gpu_ctx, sc, W, H, 16, scenes.SEED)
    st = Settings(scenes.camera(W, H), 16)  # the shipped defaults
    guided = dict(radius=st.denoise_radius, patch_radius=st.denoise_patch, k=st.denoise_k, alpha=st.denoise_alpha, k_f=st.denoise_feature_k,
                  tau=st.denoise_feature_tau)
    un = tgd.rmse(render.denoise_arrays(gpu_ctx, S, Q, [(0, 0, W, H)], [16]), ref)
    gd = tgd.rmse(render.denoise_guided_arrays(gpu_ctx, S, Q, F, G, [(0, 0, W, H)], [16], **guided), ref)
    print("guided quality: %s 256x144 16 spp: RMSE unguided %.5g guided %.5g ratio %.4f" % (which, un, gd, gd / un))
    F_a, G_a = _feature_sums(gpu_ctx, sc, W, H, 2048, 0x1234567)
    den = render.denoise_guided_arrays(gpu_ctx, S_a, Q_a, F_a, G_a, [(0, 0, W, H)], [2048], **guided)
    conv = tgd.rmse(den, ref_b) / tgd.rmse(ref, ref_b)
    print("guided quality: %s converged frame ratio %.4f" % (which, conv))
    assert gd <= un, (gd, un)
    assert conv <= 1.05, conv
