"""rmd_denoise_atrous on the device: the kernels against the numpy restatement (tests/denoise_atrous_ref.py), the definition's exact properties,
the step edge, the host paths that use it (Python render_tiled / await_, the C++ mirror through raymond_cli), and its quality on real renders."""
import os
import subprocess

import numpy as np
import pytest

import denoise_atrous_ref as aref
import denoise_guided_ref as gref
import denoise_ref
import test_gpu_denoise as tgd
import test_gpu_denoise_guided as tgg
from raymond_amd import render, scenes
from raymond_amd.scene import Settings, generate_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEVELS = (0, 1, 2, 3, 5, 8)
K_ALPHA = ((3.0, 1.0), (0.45, 0.5), (6.0, 0.0))
MODES = {"unguided": None, "guided": (1.0, 1e-2), "guided_paper": (0.6, 1e-3)}


# ---------------------------------------------------------------- 1. the kernels against the restatement
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("W,H", [(1, 1), (5, 200), (37, 23), (64, 48), (200, 120)])
def test_kernel_matches_the_restatement(gpu_ctx, W, H, mode):
    """test_gpu_denoise.py's recipe (counts of 0 and 1, an uncovered tile, NaN / +-inf in S, inf in Q; NaN / inf in F and G when guided) and its
    criterion, for every pixel: the definition has no discrete decision.  The frames are narrower than a wave, than a workgroup's tile and than
    twice the largest step, and 200 x 120 has room for step 16; at 8 levels the last steps leave the frame and only the centre tap remains."""
    rng = np.random.default_rng(W * 1000 + H)
    rects, counts = tgd._tiles_with_counts(W, H, 8, 16, rng) if W * H > 1 else ([(0, 0, 1, 1)], [9])
    n_img = denoise_ref.count_image(W, H, rects, counts)
    S, Q = tgd._moments(rng, n_img)
    F, G = tgg._features(rng, n_img)
    if W * H > 1:
        tgd._poison(S, Q, rng)
    guide = {} if MODES[mode] is None else dict(k_f=MODES[mode][0], tau=MODES[mode][1])
    for k, alpha in K_ALPHA:
        refs = aref.atrous_all(S, Q, n_img, LEVELS, k=k, alpha=alpha, F=F if guide else None, G=G if guide else None, **guide)
        for levels in LEVELS:
            dev = render.denoise_atrous_arrays(gpu_ctx, S, Q, F if guide else None, G if guide else None, rects, counts, levels=levels, k=k, alpha=alpha, **guide)
            tgd._agree(dev, refs[levels])
    if guide and W * H > 100:  # the features mattered
        assert not np.array_equal(refs[3], aref.atrous(S, Q, n_img, levels=3, k=k, alpha=alpha), equal_nan=True)


# ---------------------------------------------------------------- 2. bit-exact properties
def _poisoned_frame(seed, W, H, tw, th, min_count=0):
    rng = np.random.default_rng(seed)
    rects, counts = tgd._tiles_with_counts(W, H, tw, th, rng)
    counts = [max(c, min_count) for c in counts]
    n_img = denoise_ref.count_image(W, H, rects, counts)
    S, Q = tgd._moments(rng, n_img)
    tgd._poison(S, Q, rng)
    return S, Q, rects, counts, n_img


def test_levels_zero_is_the_mean_bit_for_bit(gpu_ctx):
    S, Q, rects, counts, n_img = _poisoned_frame(3, 45, 29, 16, 8)
    S[3, 3] = -0.0  # -0.0 / n stays -0.0
    with np.errstate(all="ignore"):
        mean = S / n_img[..., None].astype(np.float64)
    F, G = tgg._features(np.random.default_rng(4), n_img)
    assert render.denoise_atrous_arrays(gpu_ctx, S, Q, None, None, rects, counts, levels=0).tobytes() == mean.tobytes()
    assert render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, rects, counts, levels=0).tobytes() == mean.tobytes()
    assert np.isnan(mean).any() and np.isinf(mean).any()


@pytest.mark.parametrize("levels", [1, 3, 5])
def test_null_features_equal_zero_features(gpu_ctx, levels):
    S, Q, rects, counts, _ = _poisoned_frame(11, 70, 41, 16, 8, min_count=2)  # counts >= 2: every covered pixel's zero features are valid
    Z = np.zeros((41, 70, 7))
    null = render.denoise_atrous_arrays(gpu_ctx, S, Q, None, None, rects, counts, levels=levels, k_f=float("nan"), tau=-1.0)
    zero = render.denoise_atrous_arrays(gpu_ctx, S, Q, Z, Z, rects, counts, levels=levels)
    assert null.tobytes() == zero.tobytes()
    assert np.isfinite(null).any() and np.isnan(null).any()


def test_one_rect_equals_tiles_at_the_same_count_and_repeats(gpu_ctx):
    rng = np.random.default_rng(6)
    W, H, n = 77, 53, 12
    S, Q, rect, count = tgd._plain_frame(rng, W, H, n)
    F, G = tgg._features(rng, np.full((H, W), n))
    tiles = generate_tiles(W, H, (32, 32))
    for feats in ((None, None), (F, G)):
        one = render.denoise_atrous_arrays(gpu_ctx, S, Q, *feats, rect, count)
        many = render.denoise_atrous_arrays(gpu_ctx, S, Q, *feats, tiles, [n] * len(tiles))
        again = render.denoise_atrous_arrays(gpu_ctx, S, Q, *feats, tiles, [n] * len(tiles))
        assert one.tobytes() == many.tobytes() == again.tobytes()
        assert np.isfinite(one).all()


def test_the_output_buffer_written_twice_gives_the_same_bits(gpu_ctx):
    rng = np.random.default_rng(7)
    W, H, n = 33, 31, 5
    S, Q, rect, count = tgd._plain_frame(rng, W, H, n)
    fbs = [render.Framebuffer(gpu_ctx, W, H) for _ in range(3)]
    try:
        fbs[0].upload(S)
        fbs[1].upload(Q)
        render.denoise_atrous(gpu_ctx, fbs[0], fbs[1], rect, count, fbs[2], levels=4)
        first = fbs[2].download()
        render.denoise_atrous(gpu_ctx, fbs[0], fbs[1], rect, count, fbs[2], levels=4)
        assert fbs[2].download().tobytes() == first.tobytes()
        assert fbs[0].download().tobytes() == S.tobytes() and fbs[1].download().tobytes() == Q.tobytes()  # the inputs are untouched
    finally:
        for fb in fbs:
            fb.close()
    tgd._agree(first, aref.atrous(S, Q, np.full((H, W), n), levels=4))


def test_a_nan_pixel_stays_nan_and_does_not_spread(gpu_ctx):
    """The construction of test_gpu_denoise.py: the pixel made invalid through a NaN gives every other pixel the bytes it gets when the pixel is
    made invalid through a 1 x 1 rect of count 1."""
    rng = np.random.default_rng(5)
    W, H, n = 48, 40, 16
    S, Q, _, _ = tgd._plain_frame(rng, W, H, n)
    px, py = 20, 17
    tiles = generate_tiles(W, H, (8, 8))
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
    by_count = render.denoise_atrous_arrays(gpu_ctx, S, Q, None, None, [r for r, _ in split], [c for _, c in split])
    S_nan = S.copy()
    S_nan[py, px, 1] = np.nan
    by_nan = render.denoise_atrous_arrays(gpu_ctx, S_nan, Q, None, None, tiles, [n] * len(tiles))
    assert np.isnan(by_nan[py, px, 1])
    mask = np.ones((H, W), dtype=bool)
    mask[py, px] = False
    assert np.isfinite(by_nan[mask]).all()
    assert by_nan[mask].tobytes() == by_count[mask].tobytes()
    plain = render.denoise_atrous_arrays(gpu_ctx, S, Q, None, None, tiles, [n] * len(tiles))
    assert not np.array_equal(plain[mask], by_nan[mask])  # the pixel mattered


def test_hit_miss_frame_on_the_device_is_exact(gpu_ctx):
    S, Q, F, G, n, u = gref.hit_miss_frame()
    H, W = n.shape
    rect, count = [(0, 0, W, H)], [int(n[0, 0])]
    for levels in (1, 2, 5, 8):
        gd = render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, rect, count, levels=levels)
        assert gd.tobytes() == u.tobytes(), levels
        un = render.denoise_atrous_arrays(gpu_ctx, S, Q, None, None, rect, count, levels=levels)
        assert un.tobytes() != u.tobytes(), levels


# ---------------------------------------------------------------- 3. the step edge
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_step_edge_on_the_device(gpu_ctx, seed):
    """The host test's two bars, at the defaults."""
    S, Q, F, G, n, truth = gref.step_edge_frame(seed)
    H, W = n.shape
    rect, count = [(0, 0, W, H)], [int(n[0, 0])]
    un = render.denoise_atrous_arrays(gpu_ctx, S, Q, None, None, rect, count)
    gd = render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, rect, count)
    ru, rg = gref.band_rmse(un, truth), gref.band_rmse(gd, truth)
    fu, fg, f0 = tgd.rmse(un, truth), tgd.rmse(gd, truth), tgd.rmse(S / n[..., None], truth)
    print("step edge on the device, seed %d: band RMSE unguided %.4f guided %.4f ratio %.3f; frame RMSE unfiltered %.4f unguided %.4f guided %.4f"
          % (seed, ru, rg, rg / ru, f0, fu, fg))
    assert rg < 0.5 * ru
    assert fu < 0.2 * f0 and fg < 0.2 * f0


# ---------------------------------------------------------------- 4. the host paths
def _scene(which):
    return scenes.reflective_spheres() if which == "spheres" else scenes.gold_dragon_standin(n=12)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_render_tiled_with_the_setting_equals_the_direct_call(gpu_ctx, which, guided):
    W, H, spp = 96, 64, 12
    sc = _scene(which)
    kw = dict(sample_count=spp, tile_size=(32, 32), bounce_limit=4, seed=scenes.SEED, samples_per_iteration=4, denoise=True, denoise_radius=5, denoise_patch=2,
              denoise_alpha=0.75, denoise_features=guided, denoise_feature_k=0.8, denoise_feature_tau=2e-3)
    st = Settings(scenes.camera(W, H), denoise_atrous=True, denoise_atrous_levels=4, denoise_atrous_k=2.5, **kw)
    handle = render.render_tiled(sc, st, devices=(0,))
    tiles = tgd._finished_tiles(handle)
    assert len(tiles) == len(generate_tiles(W, H, (32, 32)))
    S, Q, rects, counts = tgd._assemble(tiles, W, H)
    F, G = tgg._direct_features(gpu_ctx, sc, st, rects, counts) if guided else (None, None)
    expected = render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, rects, counts, levels=4, k=2.5, alpha=0.75, k_f=0.8, tau=2e-3)
    got = handle.await_()
    assert got.tobytes() == expected.tobytes()
    assert np.isfinite(got).all()
    if guided:
        assert F.any() and got.tobytes() != render.denoise_atrous_arrays(gpu_ctx, S, Q, None, None, rects, counts, levels=4, k=2.5, alpha=0.75).tobytes()
    # the setting off: the frame the render gave before the setting existed
    off = Settings(scenes.camera(W, H), **kw)
    plain = render.render_tiled(sc, off, devices=(0,))
    plain.async_await()
    params = dict(radius=5, patch_radius=2, k=0.45, alpha=0.75)
    before = (render.denoise_guided_arrays(gpu_ctx, S, Q, F, G, rects, counts, k_f=0.8, tau=2e-3, **params) if guided
              else render.denoise_arrays(gpu_ctx, S, Q, rects, counts, **params))
    assert plain.await_().tobytes() == before.tobytes()
    assert before.tobytes() != got.tobytes()


def _cli():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return tgd.CLI


@pytest.mark.parametrize("which,extra", [("spheres", []), ("spheres", ["--denoise-features", "1", "--denoise-atrous-levels", "3", "--denoise-atrous-k", "2"]),
                                         ("mesh", ["--denoise-features", "1"]), ("mesh", ["--denoise-atrous-levels", "8"])])
def test_cli_equals_the_python_path(gpu_ctx, tmp_path, which, extra):
    cli = _cli()
    W, H, spp, bounces = 96, 64, 12, 4
    ppm, raw = tmp_path / "o.ppm", tmp_path / "o.f64"
    os.environ["RAYMOND_REHEARSE_ON_DEVICE0"] = "1"
    try:
        r = subprocess.run([cli, "render", "spheres" if which == "spheres" else "dragon:12", str(W), str(H), str(spp), str(bounces), str(ppm), "--raw", str(raw),
                            "--spi", "4", "--denoise", "1", "--denoise-atrous", "1", *extra], capture_output=True, text=True)
    finally:
        os.environ.pop("RAYMOND_REHEARSE_ON_DEVICE0", None)
    assert r.returncode == 0, r.stderr
    img_cpp = np.fromfile(raw).reshape(H, W, 3)
    opts = dict(zip(extra[0::2], extra[1::2]))
    st = Settings(scenes.camera(W, H), sample_count=spp, tile_size=(32, 32), bounce_limit=bounces, seed=scenes.SEED, samples_per_iteration=4, denoise=True,
                  denoise_atrous=True, denoise_features="--denoise-features" in opts, denoise_atrous_levels=int(opts.get("--denoise-atrous-levels", 5)),
                  denoise_atrous_k=float(opts.get("--denoise-atrous-k", 3.0)))
    handle = render.render_tiled(_scene(which), st, devices=(0,))
    handle.async_await()
    img_py = handle.await_()
    assert np.isfinite(img_py).all()
    assert img_cpp.tobytes() == img_py.tobytes()


# ---------------------------------------------------------------- 5. quality on real renders
@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_quality_at_16_spp_at_the_defaults(gpu_ctx, which):
    """256 x 144, 16 spp against 2,048 spp of seed + 1, RMSE in linear radiance, the shipped defaults (5 levels, k 3.0; guided: k_f 1.0, tau 1e-2).
    Hard condition on both scenes: the filtered frame is closer to the converged one than the unfiltered mean is.  On ReflectiveSpheres also: no
    worse than rmd_denoise at its defaults on the same sums — the restatement meets that bar on the CPU at this size with the oracle's samples
    (unguided 0.0234, guided 0.0221 against denoise_ref's 0.0247; unfiltered 0.1068).  The mesh scene's ratio is printed, not asserted."""
    W, H = 256, 144
    sc = scenes.reflective_spheres() if which == "spheres" else scenes.gold_dragon_standin(n=24)
    S_ref, _ = tgd.render_moments(gpu_ctx, sc, W, H, 2048, seed=scenes.SEED + 1)
    ref = S_ref / 2048.0
    S, Q = tgd.render_moments(gpu_ctx, sc, W, H, 16, seed=scenes.SEED)
    F, G = tgg._feature_sums(gpu_ctx, sc, W, H, 16, scenes.SEED)
    rect, count = [(0, 0, W, H)], [16]
    st = Settings(scenes.camera(W, H), 16)  # the shipped defaults
    params = dict(levels=st.denoise_atrous_levels, k=st.denoise_atrous_k, alpha=st.denoise_alpha)
    noisy = tgd.rmse(S / 16.0, ref)
    un = tgd.rmse(render.denoise_atrous_arrays(gpu_ctx, S, Q, None, None, rect, count, **params), ref)
    gd = tgd.rmse(render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, rect, count, k_f=st.denoise_feature_k, tau=st.denoise_feature_tau, **params), ref)
    nlm = tgd.rmse(render.denoise_arrays(gpu_ctx, S, Q, rect, count), ref)
    print("atrous quality: %s 256x144 16 spp: RMSE unfiltered %.5g, a-trous unguided %.5g guided %.5g, rmd_denoise %.5g; ratios to rmd_denoise %.4f %.4f"
          % (which, noisy, un, gd, nlm, un / nlm, gd / nlm))
    assert un < noisy and gd < noisy, (un, gd, noisy)
    if which == "spheres":
        assert un <= 1.0 * nlm and gd <= 1.0 * nlm, (un, gd, nlm)
