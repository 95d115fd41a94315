"""rmd_denoise_atrous_dual on the device: the kernels against the numpy restatement (tests/denoise_atrous_dual_ref.py), the definition's exact
properties, the host paths that use it (Python render_tiled / await_ and its adaptive check, the C++ mirror through raymond_cli), and its quality
and its ranking of tiles on real renders."""
import os
import subprocess

import numpy as np
import pytest

import denoise_atrous_dual_ref as adref
import denoise_dual_ref
import denoise_ref
import test_gpu_denoise as tgd
from raymond_amd import render, scenes
from raymond_amd.scene import Settings, generate_tiles
from test_gpu_denoise_atrous import K_ALPHA, LEVELS, MODES
from test_gpu_denoise_dual import CLI, _assemble_dual, _cli, _two_halves
from test_gpu_denoise_dual_guided import _direct_features, _features
from test_gpu_denoise_dual_region import _bits, _random_bytes

pytestmark = pytest.mark.gpu


def _agree_err(err, f_a, f_b, dual):
    """err against the restatement's, judged relative to the values whose difference it is.  test_gpu_denoise._agree allows each filtered value
    d = 1e-9 |f| + 1e-12 max|f|; h_c = (f_Ac - f_Bc) / 2 may then be off by t_c = (d_Ac + d_Bc) / 2, and err = mean_c h_c^2 by
    mean_c (2 |h_c| t_c + t_c^2), to which 1e-9 err is added for the operations of err itself.  NaN exactly where the pixel is not dual-valid."""
    assert np.array_equal(np.isnan(err), ~dual)
    if not dual.any():
        return
    fa, fb = f_a[dual], f_b[dual]
    scale = max(np.max(np.abs(fa)), np.max(np.abs(fb)))
    t = ((1e-9 * np.abs(fa) + 1e-12 * scale) + (1e-9 * np.abs(fb) + 1e-12 * scale)) / 2.0
    h = (fa - fb) / 2.0
    ref = (h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1] + h[:, 2] * h[:, 2]) / 3.0
    tol = (2.0 * np.abs(h) * t + t * t).sum(axis=1) / 3.0 + 1e-9 * ref
    bad = np.abs(err[dual] - ref) > tol
    assert not bad.any(), "%d err values differ, worst %.3g of its tolerance" % (bad.sum(), (np.abs(err[dual] - ref) / tol).max())


class _Buffers:
    """The two halves and the features uploaded once; out and err re-filled with random bytes before each call."""

    def __init__(self, ctx, halves, F=None, G=None, seed=1):
        self.ctx, self.rng = ctx, np.random.default_rng(seed)
        H, W = halves[0].shape[:2]
        self.shape = (H, W)
        self.fbs = [render.Framebuffer(ctx, W, H) for _ in range(5)]
        self.err = render.ErrorImage(ctx, W, H)
        self.feat = [None, None]
        for fb, arr in zip(self.fbs, halves):
            fb.upload(arr)
        if F is not None:
            self.feat = [render.FeatureBuffer(ctx, W, H), render.FeatureBuffer(ctx, W, H)]
            self.feat[0].upload(F), self.feat[1].upload(G)

    def run(self, rects, counts_a, counts_b, counts_f=None, guided=False, with_err=True, **params):
        H, W = self.shape
        self.fbs[4].upload(_random_bytes(self.rng, (H, W, 3))), self.err.upload(_random_bytes(self.rng, (H, W)))
        kw = dict(features=self.feat[0], features_sq=self.feat[1], counts_f=counts_f) if guided else {}
        render.denoise_atrous_dual(self.ctx, (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3]), rects, counts_a, counts_b, self.fbs[4],
                                   self.err if with_err else None, **kw, **params)
        return self.fbs[4].download(), self.err.download()

    def close(self):
        for b in self.fbs + [self.err] + [f for f in self.feat if f is not None]:
            b.close()


def _inputs(W, H):
    rng = np.random.default_rng(W * 1000 + H + 23)
    halves, rects, counts_a, counts_b, n_a, n_b = _two_halves(rng, W, H)  # poisoned sums, unequal counts with 0 and 1, one tile uncovered
    F, G, counts_f, n_f = _features(rng, W, H, rects)  # NaN / inf among them, counts of their own (a 0 and a 1 where there are 8 rects)
    return halves, rects, counts_a, counts_b, n_a, n_b, F, G, counts_f, n_f


# ---------------------------------------------------------------- 1. the kernels against the restatement
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("W,H", [(1, 1), (5, 200), (37, 23), (64, 48), (200, 120)])
def test_kernel_matches_the_restatement(gpu_ctx, W, H, mode):
    """test_gpu_denoise.py's poisoned recipe on both halves independently and its criterion for `out`, for every pixel; `err` by _agree_err.  The
    frames are narrower than a wave, than a workgroup's tile and than twice the largest step, and 200 x 120 has room for step 16 — there (3.0, 1.0)
    alone, every (k, alpha) on the smaller frames."""
    halves, rects, counts_a, counts_b, n_a, n_b, F, G, counts_f, n_f = _inputs(W, H)
    guide = {} if MODES[mode] is None else dict(k_f=MODES[mode][0], tau=MODES[mode][1])
    ref_guide = dict(F=F, G=G, n_f=n_f, **guide) if guide else {}
    bufs = _Buffers(gpu_ctx, halves, F if guide else None, G if guide else None)
    try:
        for k, alpha in (K_ALPHA[:1] if W * H > 10000 else K_ALPHA):
            refs, dual = adref.filtered_halves_all(*halves, n_a, n_b, LEVELS, k=k, alpha=alpha, **ref_guide)
            for levels in LEVELS:
                out, err = bufs.run(rects, counts_a, counts_b, counts_f, guided=bool(guide), levels=levels, k=k, alpha=alpha, **guide)
                f_a, f_b = refs[levels]
                out_ref, _ = denoise_dual_ref.combine(f_a, f_b, halves[0], halves[2], n_a, n_b, dual)
                tgd._agree(out, out_ref)
                _agree_err(err, f_a, f_b, dual)
        if W * H > 100:
            assert dual.any() and not dual.all()
            if guide:  # the features mattered
                plain, _ = adref.filtered_halves_all(*halves, n_a, n_b, [3], k=k, alpha=alpha)
                assert not np.array_equal(refs[3][0][dual], plain[3][0][dual])
    finally:
        bufs.close()


# ---------------------------------------------------------------- 2. bit-exact properties
def test_levels_zero_is_the_closed_form_bit_for_bit(gpu_ctx):
    halves, rects, counts_a, counts_b, n_a, n_b, F, G, counts_f, n_f = _inputs(45, 29)
    S_a, Q_a, S_b, Q_b = halves
    na, nb = n_a.astype(np.float64)[..., None], n_b.astype(np.float64)[..., None]
    _, _, dual = adref.filtered_halves(*halves, n_a, n_b, levels=0)
    with np.errstate(all="ignore"):
        u_a, u_b = S_a / na, S_b / nb
        out_x = np.where(dual[..., None], (na * u_a + nb * u_b) / (na + nb), (S_a + S_b) / (na + nb))
        h = (u_a - u_b) / 2.0
        err_x = np.where(dual, (h[..., 0] * h[..., 0] + h[..., 1] * h[..., 1] + h[..., 2] * h[..., 2]) / 3.0, np.nan)
    bufs = _Buffers(gpu_ctx, halves, F, G)
    try:
        for guided in (False, True):
            out, err = bufs.run(rects, counts_a, counts_b, counts_f, guided=guided, levels=0)
            assert np.array_equal(np.isnan(out), np.isnan(out_x)) and np.array_equal(np.isnan(err), ~dual)  # (a NaN's payload is not part of the definition)
            assert out[~np.isnan(out_x)].tobytes() == out_x[~np.isnan(out_x)].tobytes() and err[dual].tobytes() == err_x[dual].tobytes()
    finally:
        bufs.close()
    assert dual.any() and not dual.all()


@pytest.mark.parametrize("n", [8, 12])
def test_equal_halves_give_the_device_rmd_denoise_atrous_and_no_error(gpu_ctx, n):
    """A == B and rect_counts_f equal to their counts: both passes take rmd_denoise_atrous's operations, so f_A = f_B = its bytes and err = 0;
    out = (n f + n f) / (2 n) is f again at n = 8 and within one rounding of it at n = 12."""
    rng = np.random.default_rng(31 + n)
    W, H = 70, 41
    rects = generate_tiles(W, H, (16, 8))
    counts = [n] * len(rects)
    counts[3] = 1  # a tile that is not valid in either half
    n_img = denoise_ref.count_image(W, H, rects, counts)
    S, Q = tgd._moments(rng, n_img)
    tgd._poison(S, Q, rng)
    F, G, _, _ = _features(rng, W, H, rects, counts_f=counts)
    bufs = _Buffers(gpu_ctx, (S, Q, S, Q), F, G)
    try:
        for levels in (1, 3, 5):
            for guided in (False, True):
                out, err = bufs.run(rects, counts, counts, counts, guided=guided, levels=levels)
                single = render.denoise_atrous_arrays(gpu_ctx, S, Q, F if guided else None, G if guided else None, rects, counts, levels=levels)
                dual = ~np.isnan(err)
                assert dual.any() and not dual.all() and np.all(err[dual] == 0.0)
                if n == 8:
                    assert out[dual].tobytes() == single[dual].tobytes(), (levels, guided)
                else:
                    assert np.all(np.abs(out[dual] - single[dual]) <= np.spacing(np.abs(single[dual]))), (levels, guided)
    finally:
        bufs.close()


@pytest.mark.parametrize("levels", [1, 3, 5])
def test_null_features_equal_zero_features(gpu_ctx, levels):
    halves, rects, counts_a, counts_b, n_a, n_b, _, _, _, _ = _inputs(70, 41)
    Z = np.zeros((41, 70, 7))
    bufs = _Buffers(gpu_ctx, halves, Z, Z)
    try:
        null = bufs.run(rects, counts_a, counts_b, None, guided=False, levels=levels, k_f=float("nan"), tau=-1.0)
        zero = bufs.run(rects, counts_a, counts_b, [max(a + b, 2) for a, b in zip(counts_a, counts_b)], guided=True, levels=levels)
        assert np.array_equal(_bits(null[0]), _bits(zero[0])) and np.array_equal(_bits(null[1]), _bits(zero[1]))
        assert np.isfinite(null[1]).any() and np.isnan(null[1]).any()
    finally:
        bufs.close()


def test_one_rect_equals_tiles_repeats_and_needs_no_error_image(gpu_ctx):
    rng = np.random.default_rng(6)
    W, H, na, nb = 77, 53, 12, 7
    S_a, Q_a, rect, _ = tgd._plain_frame(rng, W, H, na)
    S_b, Q_b, _, _ = tgd._plain_frame(rng, W, H, nb)
    tiles = generate_tiles(W, H, (32, 32))
    F, G, _, _ = _features(rng, W, H, rect, counts_f=[na + nb])
    bufs = _Buffers(gpu_ctx, (S_a, Q_a, S_b, Q_b), F, G)
    try:
        for guided in (False, True):
            one = bufs.run(rect, [na], [nb], [na + nb], guided=guided)
            many = bufs.run(tiles, [na] * len(tiles), [nb] * len(tiles), [na + nb] * len(tiles), guided=guided)
            again = bufs.run(tiles, [na] * len(tiles), [nb] * len(tiles), [na + nb] * len(tiles), guided=guided)
            for x, y in ((one, many), (many, again)):
                assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(_bits(x[1]), _bits(y[1]))
            assert np.isfinite(one[0]).all() and np.isfinite(one[1]).all()  # (the features' NaN / inf only make pixels feature-invalid)
            # err_dev = NULL: out is the same, and the error image keeps the random bytes it held
            before = _random_bytes(bufs.rng, (H, W))
            bufs.err.upload(before)
            H_, W_ = bufs.shape
            bufs.fbs[4].upload(_random_bytes(bufs.rng, (H_, W_, 3)))
            kw = dict(features=bufs.feat[0], features_sq=bufs.feat[1], counts_f=[na + nb]) if guided else {}
            render.denoise_atrous_dual(gpu_ctx, (bufs.fbs[0], bufs.fbs[1]), (bufs.fbs[2], bufs.fbs[3]), rect, [na], [nb], bufs.fbs[4], None, **kw)
            assert np.array_equal(_bits(bufs.fbs[4].download()), _bits(one[0]))
            assert np.array_equal(_bits(bufs.err.download()), _bits(before))
        for fb, arr in zip(bufs.fbs[:4], (S_a, Q_a, S_b, Q_b)):  # the inputs are untouched
            assert fb.download().tobytes() == arr.tobytes()
    finally:
        bufs.close()


def test_a_nan_pixel_stays_nan_and_does_not_spread(gpu_ctx):
    """test_gpu_denoise.py's construction: the pixel made invalid through a NaN in half A gives every other pixel the bytes it gets when the pixel is
    made invalid through a 1 x 1 rect of count 1 in half A."""
    rng = np.random.default_rng(5)
    W, H, n = 48, 40, 16
    S_a, Q_a, _, _ = tgd._plain_frame(rng, W, H, n)
    S_b, Q_b, _, _ = tgd._plain_frame(rng, W, H, n)
    px, py = 20, 17
    tiles = generate_tiles(W, H, (8, 8))
    split = []
    for (l, t, w, h) in tiles:
        if l <= px < l + w and t <= py < t + h:
            split += [((x, y, 1, 1), n) for y in range(t, t + h) for x in range(l, l + w) if (x, y) != (px, py)]
            split.append(((px, py, 1, 1), 1))
        else:
            split.append(((l, t, w, h), n))
    srects, sa = [r for r, _ in split], [c for _, c in split]
    by_count = render.denoise_atrous_dual_arrays(gpu_ctx, S_a, Q_a, S_b, Q_b, srects, sa, [n] * len(srects))
    S_nan = S_a.copy()
    S_nan[py, px, 1] = np.nan
    by_nan = render.denoise_atrous_dual_arrays(gpu_ctx, S_nan, Q_a, S_b, Q_b, tiles, [n] * len(tiles), [n] * len(tiles))
    assert np.isnan(by_nan[0][py, px, 1]) and np.isnan(by_nan[1][py, px])  # the merged mean of a NaN, and no estimate
    mask = np.ones((H, W), dtype=bool)
    mask[py, px] = False
    assert np.isfinite(by_nan[0][mask]).all() and np.isfinite(by_nan[1][mask]).all()
    assert by_nan[0][mask].tobytes() == by_count[0][mask].tobytes() and by_nan[1][mask].tobytes() == by_count[1][mask].tobytes()
    plain = render.denoise_atrous_dual_arrays(gpu_ctx, S_a, Q_a, S_b, Q_b, tiles, [n] * len(tiles), [n] * len(tiles))
    assert not np.array_equal(plain[0][mask], by_nan[0][mask])  # the pixel mattered


# ---------------------------------------------------------------- 3. the host paths
HW, HH, HSPP, HSPI, HBOUNCES = 96, 64, 32, 8, 4
HFILTER = dict(levels=4, k=2.5, alpha=0.75)
HGUIDE = dict(k_f=0.8, tau=2e-3)


def _scene(which):
    return scenes.reflective_spheres() if which == "spheres" else scenes.gold_dragon_standin(n=24)


def _settings(**kw):
    return Settings(scenes.camera(HW, HH), sample_count=HSPP, tile_size=(32, 32), bounce_limit=HBOUNCES, seed=scenes.SEED, samples_per_iteration=HSPI,
                    denoise=True, denoise_dual=True, denoise_alpha=0.75, denoise_atrous_levels=4, denoise_atrous_k=2.5, denoise_feature_k=0.8,
                    denoise_feature_tau=2e-3, **kw)


CLI_ARGS = ["--denoise", "1", "--denoise-dual", "1", "--denoise-dual-atrous", "1", "--denoise-alpha", "0.75", "--denoise-atrous-levels", "4", "--denoise-atrous-k", "2.5",
            "--denoise-feature-k", "0.8", "--denoise-feature-tau", "0.002"]


def _run_cli(tmp_path, which, extra):
    cli = _cli()
    assert os.path.samefile(cli, CLI)
    ppm, raw = tmp_path / "o.ppm", tmp_path / "o.f64"
    r = subprocess.run([cli, "render", "spheres" if which == "spheres" else "dragon:24", str(HW), str(HH), str(HSPP), str(HBOUNCES), str(ppm), "--raw", str(raw),
                        "--spi", str(HSPI), *CLI_ARGS, *extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.fromfile(raw).reshape(HH, HW, 3)


def _expected_frame(ctx, sc, handle, guided):
    """rmd_denoise_atrous_dual called directly on the finished tiles' halves (guided: with each tile's features at count_a + count_b)."""
    halves, rects, counts_a, counts_b = _assemble_dual(tgd._finished_tiles(handle), HW, HH)
    guide = {}
    if guided:
        counts_f = [a + b for a, b in zip(counts_a, counts_b)]
        plain_st = Settings(scenes.camera(HW, HH), sample_count=HSPP, bounce_limit=HBOUNCES, seed=scenes.SEED)
        ds = render.DeviceScene(ctx, sc)
        try:
            F, G = _direct_features(ctx, ds, plain_st, rects, counts_f)
        finally:
            ds.close()
        assert F.any()
        guide = dict(features=F, features_sq=G, counts_f=counts_f, **HGUIDE)
    frame, _ = render.denoise_atrous_dual_arrays(ctx, *halves, rects, counts_a, counts_b, **HFILTER, **guide)
    return frame, (halves, rects, counts_a, counts_b)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_render_tiled_with_the_setting_equals_the_direct_call_and_the_cli(gpu_ctx, which, guided, tmp_path):
    sc = _scene(which)
    handle = render.render_tiled(sc, _settings(denoise_dual_atrous=True, denoise_dual_features=guided), devices=(0,))
    expected, (halves, rects, counts_a, counts_b) = _expected_frame(gpu_ctx, sc, handle, guided)
    assert rects == generate_tiles(HW, HH, (32, 32)) and set(counts_a) == set(counts_b) == {HSPP // 2}
    got = handle.await_()
    assert got.tobytes() == expected.tobytes() and np.isfinite(got).all()
    if guided:
        assert got.tobytes() != render.denoise_atrous_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, **HFILTER)[0].tobytes()
    # the setting off: rmd_denoise_dual's frame at its own parameters, as before the setting existed
    if not guided:
        off = render.render_tiled(sc, _settings(denoise_radius=5, denoise_patch=2), devices=(0,))
        off.async_await()
        before, _ = render.denoise_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, radius=5, patch_radius=2, k=0.45, alpha=0.75)
        assert off.await_().tobytes() == before.tobytes() and before.tobytes() != got.tobytes()
    assert _run_cli(tmp_path, which, ["--denoise-dual-features", "1"] if guided else []).tobytes() == got.tobytes()


@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_the_adaptive_check_calls_the_whole_frame_filter_and_finishes_tiles_early(gpu_ctx, which, tmp_path, monkeypatch):
    """A spy on the two wrappers the check goes through.  The threshold is the median rmd_tile_error_dual the check itself sees first (a first run
    under a threshold nothing meets), so that some tiles finish there and others go on."""
    sc = _scene(which)
    tiles = generate_tiles(HW, HH, (32, 32))
    calls = []
    real_filter, real_error, real_region = render.denoise_atrous_dual, render.tile_error_dual, render.denoise_dual

    def spy_filter(ctx, half_a, half_b, rects, counts_a, counts_b, out_fb, err_img=None, **kw):
        calls.append(("filter", list(rects), list(counts_a), list(counts_b), err_img, dict(kw)))
        return real_filter(ctx, half_a, half_b, rects, counts_a, counts_b, out_fb, err_img, **kw)

    def spy_error(ctx, err_img, rects):
        errors = real_error(ctx, err_img, rects)
        calls.append(("error", list(rects), err_img, [float(e) for e in errors]))
        return errors

    def spy_region(*a, **kw):
        calls.append(("nlm",))
        return real_region(*a, **kw)

    monkeypatch.setattr(render, "denoise_atrous_dual", spy_filter)
    monkeypatch.setattr(render, "tile_error_dual", spy_error)
    monkeypatch.setattr(render, "denoise_dual", spy_region)
    render.render_tiled(sc, _settings(denoise_dual_atrous=True, adaptive_denoised_threshold=1e-300, adaptive_min_samples=16), devices=(0,))
    assert [c[0] for c in calls] == ["filter", "error"] and calls[0][1] == tiles  # one check, at 16 of 32 samples (24 is an odd number of passes)
    threshold = float(np.median(calls[1][3]))
    del calls[:]
    st = _settings(denoise_dual_atrous=True, adaptive_denoised_threshold=threshold, adaptive_min_samples=16)
    handle = render.render_tiled(sc, st, devices=(0,))
    assert [c[0] for c in calls] == ["filter", "error"]
    kind, rects, counts_a, counts_b, err_img, kw = calls[0]
    assert rects == tiles and counts_a == counts_b == [HSPI] * len(tiles) and err_img is calls[1][2]  # the whole frame, into the image the errors come from
    assert kw == dict(levels=4, k=2.5, alpha=0.75)
    assert calls[1][1] == tiles  # every tile was live
    fin = tgd._finished_tiles(handle)
    early = [(t.left, t.top, t.width, t.height) for t in fin if t.sample_count == 2 * HSPI]
    assert early == [r for r, e in zip(tiles, calls[1][3]) if e <= threshold] and 0 < len(early) < len(tiles)
    assert all(t.sample_count == HSPP for t in fin if (t.left, t.top, t.width, t.height) not in early)
    assert [t.error for t in fin if t.sample_count == 2 * HSPI] == [e for e in calls[1][3] if e <= threshold]
    print("adaptive a-trous check (%s): threshold %.6g, %d of %d tiles finished at %d samples" % (which, threshold, len(early), len(tiles), 2 * HSPI))
    del calls[:]
    expected, _ = _expected_frame(gpu_ctx, sc, handle, False)
    del calls[:]
    got = handle.await_()
    assert got.tobytes() == expected.tobytes()
    assert [c[0] for c in calls] == ["filter"] and calls[0][4] is not None  # (await_'s own call, through the arrays wrapper)
    monkeypatch.undo()
    # the C++ loop makes the same calls: the same frame, and the whole-frame entry point among its imports
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _cli()], check=True, capture_output=True, text=True).stdout
    assert "rmd_denoise_atrous_dual" in undefined
    assert _run_cli(tmp_path, which, ["--adaptive-denoised", "%.17g" % threshold, "--adaptive-min", "16"]).tobytes() == got.tobytes()


# ---------------------------------------------------------------- 4. quality and ranking on real renders
# The bars, measured on the CPU at this size with the restatement and the oracle's per-sample frames over three seeds (tools/atrous_dual_bars.py;
# DESIGN.md section 18): (a) the largest ratio plus twice the seed-to-seed spread, (b) the smallest rank correlation minus twice the spread.
# CPU, seeds SEED, SEED + 2, SEED + 3: spheres ratios 1.0269, 1.0006, 1.0240 (spread 0.0264) and correlations 0.9000, 0.8998, 0.8758 (spread 0.0242);
# mesh ratios 1.0439, 1.0390, 1.0444 (spread 0.0054) and correlations 0.8424, 0.8056, 0.8540 (spread 0.0484).
BARS = {"spheres": dict(ratio=1.0797, spearman=0.8274), "mesh": dict(ratio=1.0552, spearman=0.7089)}


def _spearman(a, b):
    def ranks(v):
        v = np.asarray(v, dtype=np.float64)
        r = np.empty(len(v))
        r[np.argsort(v, kind="stable")] = np.arange(len(v), dtype=np.float64)
        for x in np.unique(v):
            r[v == x] = r[v == x].mean()
        return r - r.mean()

    ra, rb = ranks(a), ranks(b)
    return float((ra * rb).sum() / np.sqrt((ra * ra).sum() * (rb * rb).sum()))


@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_quality_and_ranking_at_8_plus_8_spp_at_the_defaults(gpu_ctx, which):
    """256 x 144, samples [0, 8) as half A and [8, 16) as half B against 2,048 spp of seed + 1, RMSE in linear radiance, the shipped defaults (5
    levels, k 3.0, alpha 1, unguided).  Hard condition: the dual frame is closer to the converged one than the merged unfiltered mean is.  (a) its
    RMSE over rmd_denoise_atrous's on the merged sums and (b) Spearman's rank correlation over the 32 x 32 tiles between rmd_tile_error_dual of err
    and the tile's true RMS error are held to BARS.  rmd_denoise_dual's two figures on the same halves are printed for comparison."""
    W, H, half = 256, 144, 8
    sc = scenes.reflective_spheres() if which == "spheres" else scenes.gold_dragon_standin(n=24)
    tiles = generate_tiles(W, H, (32, 32))
    ref = tgd.render_moments(gpu_ctx, sc, W, H, 2048, seed=scenes.SEED + 1)[0] / 2048.0
    st = Settings(scenes.camera(W, H), sample_count=2 * half, bounce_limit=5, seed=scenes.SEED)  # the shipped defaults
    ds = render.DeviceScene(gpu_ctx, sc)
    fbs = [render.Framebuffer(gpu_ctx, W, H) for _ in range(5)]
    err_img = render.ErrorImage(gpu_ctx, W, H)
    try:
        for j in range(2):
            render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fbs[2 * j], j * half, half, framebuffer_sq=fbs[2 * j + 1])
        S_a, Q_a, S_b, Q_b = (fb.download() for fb in fbs[:4])
        c = [half] * len(tiles)
        params = dict(levels=st.denoise_atrous_levels, k=st.denoise_atrous_k, alpha=st.denoise_alpha)
        render.denoise_atrous_dual(gpu_ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), tiles, c, c, fbs[4], err_img, **params)
        out, terr = fbs[4].download(), render.tile_error_dual(gpu_ctx, err_img, tiles)
        render.denoise_dual(gpu_ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), tiles, c, c, fbs[4], err_img)
        nlm, nlm_terr = fbs[4].download(), render.tile_error_dual(gpu_ctx, err_img, tiles)
    finally:
        for o in fbs + [err_img, ds]:
            o.close()
    single = render.denoise_atrous_arrays(gpu_ctx, S_a + S_b, Q_a + Q_b, None, None, tiles, [2 * half] * len(tiles), **params)

    def true_rms(img):
        return [tgd.rmse(img[t : t + h, l : l + w], ref[t : t + h, l : l + w]) for (l, t, w, h) in tiles]

    noisy, dual, one, nl = tgd.rmse((S_a + S_b) / (2.0 * half), ref), tgd.rmse(out, ref), tgd.rmse(single, ref), tgd.rmse(nlm, ref)
    rho, rho_nlm = _spearman(terr, true_rms(out)), _spearman(nlm_terr, true_rms(nlm))
    print("atrous dual quality: %s 256x144 8+8 spp: RMSE unfiltered %.5g, dual a-trous %.5g, single a-trous %.5g (ratio %.4f, bar %.4f), rmd_denoise_dual %.5g; "
          "rank correlation %.4f (bar %.4f), rmd_denoise_dual's %.4f" % (which, noisy, dual, one, dual / one, BARS[which]["ratio"], nl, rho, BARS[which]["spearman"], rho_nlm))
    assert dual < noisy, (dual, noisy)
    assert dual / one <= BARS[which]["ratio"], (dual, one)
    assert rho >= BARS[which]["spearman"], rho
