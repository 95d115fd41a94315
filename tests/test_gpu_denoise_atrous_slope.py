"""The three a-trous _slope calls on the device (rmd_denoise_atrous_slope, rmd_denoise_atrous_dual_slope and its region form): the kernels against the
numpy restatement (tests/denoise_atrous_slope_ref.py) for every pixel, the slope planes bit for bit, every bit-exact consequence of the definition with
no tolerance, the region form against the whole-frame call with no tolerance, the host paths (Python render_tiled / await_, the adaptive dual loop with
and without the region setting, the C++ mirror through raymond_cli), and the quality on rendered frames against rmd_denoise_atrous.

The frames, counts, poison and tolerances are test_gpu_denoise.py's, test_gpu_denoise_atrous_dual.py's and test_gpu_denoise_slope.py's own."""
import subprocess

import numpy as np
import pytest

import denoise_atrous_dual_region_ref as rref
import denoise_atrous_slope_ref as asref
import denoise_dual_guided_ref as dgref
import denoise_dual_ref
import denoise_guided_ref as gref
import denoise_ref
import denoise_slope_ref as slref
import test_gpu_denoise as tgd
import test_gpu_denoise_atrous_dual as tgad
import test_gpu_denoise_guided as tgg
from raymond_amd import probe, render, scenes
from raymond_amd.scene import Settings, generate_tiles
from test_gpu_denoise_dual import _assemble_dual, _cli
from test_gpu_denoise_dual_guided import _direct_features
from test_gpu_denoise_dual_region import _bits, _expect, _mask, _message_key, _random_bytes
from test_gpu_denoise_slope import _inputs

pytestmark = pytest.mark.gpu

# 37 x 23: narrower than one 64-wide workgroup row, odd both ways, and at 5 levels the taps leave the frame on both sides; 70 x 41: one full and one
# partial 64-column block and a partial 4-row block
SHAPES = [(37, 23), (70, 41)]
LEVELS = (0, 1, 3, 5)
SLOPES = (0.0, 3.0, 50.0)
GUIDE = dict(k_f=1.0, tau=1e-2)
_CACHE = {}


def _frame(W, H):
    """test_gpu_denoise_slope._inputs, once per shape: poisoned halves with unequal counts, features with a ramp, steps, misses and NaN / inf — a
    neighbour is missing on each axis somewhere, and the ramp reaches the frame's border."""
    if (W, H) not in _CACHE:
        _CACHE[(W, H)] = _inputs(W, H)
    return _CACHE[(W, H)]


# ---------------------------------------------------------------- the device against the restatement
@pytest.mark.parametrize("W,H", SHAPES)
def test_the_single_call_matches_the_restatement(gpu_ctx, W, H):
    _, halves, rects, counts_a, _, n_a, _, F1, G1, *_ = _frame(W, H)
    S, Q = halves[0], halves[1]
    refs = {}
    for slope in SLOPES:
        refs[slope] = asref.atrous_slope_all(S, Q, n_a, LEVELS, F=F1, G=G1, slope=slope, **GUIDE)
        for levels in LEVELS:
            dev = render.denoise_atrous_arrays(gpu_ctx, S, Q, F1, G1, rects, counts_a, levels=levels, slope=slope, **GUIDE)
            tgd._agree(dev, refs[slope][levels])
    for a, b in ((0.0, 3.0), (3.0, 50.0)):  # the slope mattered, and a larger one matters more
        assert not np.array_equal(refs[a][3], refs[b][3], equal_nan=True)


@pytest.mark.parametrize("W,H", SHAPES)
def test_the_dual_call_matches_the_restatement(gpu_ctx, W, H):
    _, halves, rects, counts_a, counts_b, n_a, n_b, _, _, F2, G2, counts_f, n_f = _frame(W, H)
    bufs = tgad._Buffers(gpu_ctx, halves, F2, G2)
    try:
        for slope in SLOPES:
            refs, dual = asref.filtered_halves_slope_all(*halves, n_a, n_b, LEVELS, F=F2, G=G2, n_f=n_f, slope=slope, **GUIDE)
            for levels in LEVELS:
                out, err = bufs.run(rects, counts_a, counts_b, counts_f, guided=True, levels=levels, slope=slope, **GUIDE)
                f_a, f_b = refs[levels]
                tgd._agree(out, denoise_dual_ref.combine(f_a, f_b, halves[0], halves[2], n_a, n_b, dual)[0])
                tgad._agree_err(err, f_a, f_b, dual)
        assert dual.any() and not dual.all()
    finally:
        bufs.close()


# ---------------------------------------------------------------- the slope planes, bit for bit
def _dual_features(halves, n_a, n_b, F, G, n_f):
    _, _, ok_a = denoise_ref.mean_and_variance(halves[0], halves[1], n_a)
    _, _, ok_b = denoise_ref.mean_and_variance(halves[2], halves[3], n_b)
    ff, _, _, fvalid = dgref.feature_planes(F, G, n_f, ok_a & ok_b, 1.0, 1e-2)
    return ff, fvalid


@pytest.mark.parametrize("W,H", SHAPES)
def test_the_whole_frame_slope_planes_are_the_restatements(gpu_ctx, W, H):
    """The whole-frame a-trous calls make their planes with feature_slope_kernel through launch_feature_slope, the launcher rmd_probe_feature_slope calls:
    the single call's f (at half A's counts) and the dual calls' f (dual-valid, own counts), every border and missing neighbour among them."""
    _, halves, _, _, _, n_a, n_b, F1, G1, F2, G2, _, n_f = _frame(W, H)
    _, _, valid = denoise_ref.mean_and_variance(halves[0], halves[1], n_a)
    ff1, _, fvalid1 = gref.feature_mean_and_variance(F1, G1, n_a, valid)
    for ff, fvalid in ((ff1, fvalid1), _dual_features(halves, n_a, n_b, F2, G2, n_f)):
        for slope in (3.0, 50.0):
            want = slref.slope_planes(ff, fvalid, slope)
            assert probe.feature_slope(gpu_ctx, ff, fvalid, slope).tobytes() == want.tobytes()
        assert (want > 0).any() and (~fvalid).any() and fvalid[0].any() and fvalid[:, 0].any()


RW, RH, RLEVELS = 96, 64, 3  # the region is dilated by 2 * (2^3 - 1) = 14: interior, border and frame-clipped parts
REGIONS = {"one_rect_off_every_alignment": [(41, 27, 5, 3)],
           "two_frame_corners": [(0, 0, 9, 6), (RW - 7, RH - 5, 7, 5)],
           "the_whole_frame_in_four": [(0, 0, 50, 30), (50, 0, RW - 50, 30), (0, 30, 50, RH - 30), (50, 30, RW - 50, RH - 30)]}


class _Region:
    """The two halves and the features of the 96 x 64 frame uploaded once."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.rng, halves, self.rects, self.counts_a, self.counts_b, self.n_a, self.n_b, _, _, self.F, self.G, self.counts_f, self.n_f = _frame(RW, RH)
        self.halves = halves
        self.fbs = [render.Framebuffer(ctx, RW, RH) for _ in range(5)]
        self.err = render.ErrorImage(ctx, RW, RH)
        self.feat = [render.FeatureBuffer(ctx, RW, RH), render.FeatureBuffer(ctx, RW, RH)]
        for fb, arr in zip(self.fbs, halves):
            fb.upload(arr)
        self.feat[0].upload(self.F), self.feat[1].upload(self.G)

    def call(self, region, **params):
        render.denoise_atrous_dual(self.ctx, (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3]), self.rects, self.counts_a, self.counts_b, self.fbs[4], self.err,
                                   features=self.feat[0], features_sq=self.feat[1], counts_f=self.counts_f, region=region, levels=RLEVELS, **GUIDE, **params)

    def run(self, region, init, **params):
        self.fbs[4].upload(init[0]), self.err.upload(init[1])
        self.call(region, **params)
        return self.fbs[4].download(), self.err.download()

    def close(self):
        for b in self.fbs + [self.err] + self.feat:
            b.close()


@pytest.fixture(scope="module")
def region_bufs(gpu_ctx):
    bufs = _Region(gpu_ctx)
    yield bufs
    bufs.close()


def test_the_region_forms_slope_planes_are_the_restatements_on_level_0s_set(gpu_ctx, region_bufs):
    """The region form makes its floors over level 0's block table only; on level 0's needed set (the region grown by 2 * (2^3 - 2) = 12, clipped) they are
    the whole frame's bits — a neighbour is present when it is inside the FRAME and feature-valid, whatever the tables hold."""
    b = region_bufs
    ff, fvalid = _dual_features(b.halves, b.n_a, b.n_b, b.F, b.G, b.n_f)
    want = slref.slope_planes(ff, fvalid, 3.0)
    for name, region in REGIONS.items():
        b.call(region, slope=3.0)
        got = probe.atrous_region_slope_planes(gpu_ctx, RW, RH)
        _, R = rref.needed_sets(region, RLEVELS, RW, RH)
        assert R[0].any() and got[R[0]].tobytes() == want[R[0]].tobytes(), name
        assert (want[R[0]] > 0).any()


# ---------------------------------------------------------------- the definition's consequences, bit for bit
@pytest.mark.parametrize("W,H", SHAPES)
def test_slope_zero_and_null_features_are_the_calls_without_the_suffix(gpu_ctx, W, H):
    rng, halves, rects, counts_a, counts_b, _, _, F1, G1, F2, G2, counts_f, _ = _frame(W, H)
    S, Q = halves[0], halves[1]
    region = [(3, 5, 20, 11), (W - 9, 0, 9, H)]
    for levels in (0, 3):
        want = render.denoise_atrous_arrays(gpu_ctx, S, Q, F1, G1, rects, counts_a, levels=levels, **GUIDE)
        assert render.denoise_atrous_arrays(gpu_ctx, S, Q, F1, G1, rects, counts_a, levels=levels, slope=0.0, **GUIDE).tobytes() == want.tobytes()
        plain = render.denoise_atrous_arrays(gpu_ctx, S, Q, None, None, rects, counts_a, levels=levels)
        assert render.denoise_atrous_arrays(gpu_ctx, S, Q, None, None, rects, counts_a, levels=levels, slope=float("nan")).tobytes() == plain.tobytes()
        init = dict(out_init=_random_bytes(rng, (H, W, 3)), err_init=_random_bytes(rng, (H, W)))
        guide = dict(features=F2, features_sq=G2, counts_f=counts_f, **GUIDE)
        for reg in (None, region):
            want = render.denoise_atrous_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, region=reg, levels=levels, **init, **guide)
            got = render.denoise_atrous_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, region=reg, levels=levels, slope=0.0, **init, **guide)
            assert _bits(got[0]).tobytes() == _bits(want[0]).tobytes() and _bits(got[1]).tobytes() == _bits(want[1]).tobytes(), (levels, reg)
            want = render.denoise_atrous_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, region=reg, levels=levels, **init)
            got = render.denoise_atrous_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, region=reg, levels=levels, slope=float("nan"), **init)
            assert _bits(got[0]).tobytes() == _bits(want[0]).tobytes() and _bits(got[1]).tobytes() == _bits(want[1]).tobytes(), (levels, reg)
    # levels = 0 is the closed form at any slope: no feature and no slope is read
    zero = render.denoise_atrous_arrays(gpu_ctx, S, Q, F1, G1, rects, counts_a, levels=0, slope=3.0, **GUIDE)
    assert zero.tobytes() == render.denoise_atrous_arrays(gpu_ctx, S, Q, None, None, rects, counts_a, levels=0).tobytes()
    a = render.denoise_atrous_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, levels=0, slope=3.0, **guide)
    b = render.denoise_atrous_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, levels=0)
    assert _bits(a[0]).tobytes() == _bits(b[0]).tobytes() and _bits(a[1]).tobytes() == _bits(b[1]).tobytes()


@pytest.mark.parametrize("frame", ["step1", "hit_miss"])
def test_features_with_a_flat_side_give_the_slope_zero_bytes_on_the_device(gpu_ctx, frame):
    S, Q, F, G, n, _ = gref.hit_miss_frame() if frame == "hit_miss" else gref.step_edge_frame(1)
    H, W = n.shape
    rect, c = [(0, 0, W, H)], [int(n[0, 0])]
    zero = render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, rect, c, slope=0.0)
    dual = dict(features=F + F, features_sq=G + G, counts_f=[2 * c[0]])
    dzero = render.denoise_atrous_dual_arrays(gpu_ctx, S, Q, S, Q, rect, c, c, slope=0.0, **dual)
    for slope in (1.0, 3.0, 50.0):
        assert render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, rect, c, slope=slope).tobytes() == zero.tobytes(), slope
        d = render.denoise_atrous_dual_arrays(gpu_ctx, S, Q, S, Q, rect, c, c, slope=slope, **dual)
        assert d[0].tobytes() == dzero[0].tobytes() and d[1].tobytes() == dzero[1].tobytes(), slope
    assert zero.tobytes() != render.denoise_atrous_arrays(gpu_ctx, S, Q, None, None, rect, c).tobytes()  # (the guide is not idle)


def test_zero_features_are_the_unguided_bytes_and_equal_halves_the_single_call(gpu_ctx):
    W, H = 70, 41
    _, halves, rects, counts_a, counts_b, *_ = _frame(W, H)
    Z = np.zeros((H, W, 7))
    twos = [max(c, 2) for c in counts_a]  # counts >= 2: every valid pixel is feature-valid; no slope, and w_f = exp(-0) = 1 cuts no weight
    S, Q = halves[0], halves[1]
    for levels in (1, 3):
        plain = render.denoise_atrous_arrays(gpu_ctx, S, Q, None, None, rects, twos, levels=levels)
        assert render.denoise_atrous_arrays(gpu_ctx, S, Q, Z, Z, rects, twos, levels=levels, slope=3.0).tobytes() == plain.tobytes() and np.isfinite(plain).any()
        want = render.denoise_atrous_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, levels=levels)
        got = render.denoise_atrous_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, levels=levels, features=Z, features_sq=Z, counts_f=[2 + i % 5 for i in range(len(rects))],
                                                slope=3.0)
        assert _bits(got[0]).tobytes() == _bits(want[0]).tobytes() and _bits(got[1]).tobytes() == _bits(want[1]).tobytes()
    # equal halves with rect_counts_f equal to their counts: the single call's bytes and err = 0 (the dome: the slope is not idle; 16 + 16 samples)
    S, Q, F, G, n = slref.dome_frame(2)[:5]
    H, W = n.shape
    rect, c = [(0, 0, W, H)], [16]
    for levels in (1, 5):
        single = render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, rect, c, levels=levels, slope=3.0)
        out, err = render.denoise_atrous_dual_arrays(gpu_ctx, S, Q, S, Q, rect, c, c, levels=levels, features=F, features_sq=G, counts_f=c, slope=3.0)
        assert out.tobytes() == single.tobytes() and np.all(err == 0.0)
    assert single.tobytes() != render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, rect, c, levels=5).tobytes()


def test_a_pixels_value_does_not_depend_on_how_the_rects_cut_the_frame(gpu_ctx):
    W, H = 70, 41
    S, Q, F, G, n = (a[:H, :W] for a in _dome_like(W, H))
    one, c1 = [(0, 0, W, H)], [16]
    for tile in ((8, 16), (32, 32)):
        tiles = generate_tiles(W, H, tile)
        cs = [16] * len(tiles)
        assert (render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, tiles, cs, levels=3, slope=3.0).tobytes()
                == render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, one, c1, levels=3, slope=3.0).tobytes())
        a = render.denoise_atrous_dual_arrays(gpu_ctx, S, Q, Q, S + Q, tiles, cs, cs, levels=3, features=F, features_sq=G, counts_f=cs, slope=3.0)
        b = render.denoise_atrous_dual_arrays(gpu_ctx, S, Q, Q, S + Q, one, c1, c1, levels=3, features=F, features_sq=G, counts_f=c1, slope=3.0)
        assert _bits(a[0]).tobytes() == _bits(b[0]).tobytes() and _bits(a[1]).tobytes() == _bits(b[1]).tobytes()


def _dome_like(W, H):
    """A frame of 16 samples a pixel whose features curve everywhere (so that the floors are not idle), of any size."""
    rng = np.random.default_rng(W * 100 + H)
    smp = 0.5 + rng.normal(0, 0.4, (16, H, W, 3))
    y, x = np.mgrid[0:H, 0:W]
    f = np.zeros((H, W, 7))
    f[..., 0], f[..., 1] = np.sin(x / 9.0), np.cos(y / 7.0)
    f[..., 2], f[..., 3:6], f[..., 6] = 0.5, 0.5, 3.0 + 0.01 * x * y
    F = f * 16.0
    return smp.sum(0), (smp * smp).sum(0), F, F * f, np.full((H, W), 16)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_dome_on_the_device(gpu_ctx, seed):
    """The host test's bars on the device's own frames: disc RMSE at slope 3 below 0.5 of slope 0's (the restatement: 0.34 - 0.37), at slope 8 below
    slope 3's."""
    S, Q, F, G, n, truth, disc = slref.dome_frame(seed)
    H, W = n.shape
    r = {s: slref.disc_rmse(render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, [(0, 0, W, H)], [16], slope=s), truth, disc) for s in (0.0, 3.0, 8.0)}
    print("dome on the device, seed %d: disc RMSE slope 0 %.5f slope 3 %.5f (x%.3f) slope 8 %.5f" % (seed, r[0.0], r[3.0], r[3.0] / r[0.0], r[8.0]))
    assert r[3.0] < 0.5 * r[0.0] and r[8.0] < r[3.0]


# ---------------------------------------------------------------- the region form: no tolerance
def test_region_equals_the_whole_frame_call_and_nothing_else_is_written(gpu_ctx, region_bufs):
    b = region_bufs
    init = (_random_bytes(b.rng, (RH, RW, 3)), _random_bytes(b.rng, (RH, RW)))  # the sentinel: random bytes, NaNs of every payload among them
    full_out, full_err = b.run(None, init, slope=3.0)
    assert np.isnan(full_err).any() and np.isfinite(full_err).any()
    assert _bits(b.run(None, init, slope=0.0)[0]).tobytes() != _bits(full_out).tobytes()  # the slope mattered
    for name, region in REGIONS.items():
        mask = _mask(RW, RH, region)
        out, err = b.run(region, init, slope=3.0)
        assert _bits(out).tobytes() == _expect(mask, full_out, init[0]).tobytes(), name
        assert _bits(err).tobytes() == _expect(mask, full_err, init[1]).tobytes(), name
    # disjoint calls compose, in both orders
    quarters = REGIONS["the_whole_frame_in_four"]
    for first, second in ((quarters[::2], quarters[1::2]), (quarters[1::2], quarters[::2])):
        b.run(first, init, slope=3.0)
        b.call(second, slope=3.0)  # into the buffers as the first call left them
        assert _bits(b.fbs[4].download()).tobytes() == _bits(full_out).tobytes() and _bits(b.err.download()).tobytes() == _bits(full_err).tobytes()


# ---------------------------------------------------------------- the host paths (96 x 64, 12 spp)
HW, HH, HSPP, HBOUNCES = 96, 64, 12, 4
HFILTER = dict(levels=4, k=2.5, alpha=0.75)
HGUIDE = dict(k_f=0.8, tau=2e-3)
HCOMMON = dict(sample_count=HSPP, tile_size=(32, 32), bounce_limit=HBOUNCES, seed=scenes.SEED, denoise=True, denoise_alpha=0.75, denoise_atrous_levels=4,
               denoise_atrous_k=2.5, denoise_feature_k=0.8, denoise_feature_tau=2e-3, denoise_atrous_slope=3.0)
HCLI = ["--denoise", "1", "--denoise-alpha", "0.75", "--denoise-atrous-levels", "4", "--denoise-atrous-k", "2.5", "--denoise-feature-k", "0.8", "--denoise-feature-tau",
        "0.002", "--denoise-atrous-slope", "3"]


def _run_cli(tmp_path, tag, extra):
    raw = tmp_path / (tag + ".f64")
    r = subprocess.run([_cli(), "render", "spheres", str(HW), str(HH), str(HSPP), str(HBOUNCES), str(tmp_path / (tag + ".ppm")), "--raw", str(raw), *HCLI, *extra],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.fromfile(raw).reshape(HH, HW, 3)


def test_render_tiled_with_the_setting_equals_the_direct_call_and_the_cli(gpu_ctx, tmp_path):
    sc = scenes.reflective_spheres()
    st = Settings(scenes.camera(HW, HH), samples_per_iteration=4, denoise_atrous=True, denoise_features=True, **HCOMMON)
    handle = render.render_tiled(sc, st, devices=(0,))
    S, Q, rects, counts = tgd._assemble(tgd._finished_tiles(handle), HW, HH)
    F, G = tgg._direct_features(gpu_ctx, sc, st, rects, counts)
    expected = render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, rects, counts, slope=3.0, **HFILTER, **HGUIDE)
    got = handle.await_()
    assert got.tobytes() == expected.tobytes() and np.isfinite(got).all()
    assert got.tobytes() != render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, rects, counts, **HFILTER, **HGUIDE).tobytes()  # the slope mattered
    assert _run_cli(tmp_path, "single", ["--spi", "4", "--denoise-atrous", "1", "--denoise-features", "1"]).tobytes() == got.tobytes()


def test_the_adaptive_dual_loop_with_and_without_the_region_setting(gpu_ctx, tmp_path, monkeypatch):
    """Passes of 2 samples, checks from 4 samples on.  The threshold is the median rmd_tile_error_dual the first check sees (a first run under a threshold
    nothing meets).  With denoise_atrous_slope every check is a _slope call — the region form's with denoise_dual_atrous_region —, and both settings send
    the same messages and give the same frame, which is rmd_denoise_atrous_dual_slope's over the finished tiles; raymond_cli writes it too."""
    sc = scenes.reflective_spheres()
    tiles = generate_tiles(HW, HH, (32, 32))
    calls = []
    real_filter, real_error = render.denoise_atrous_dual, render.tile_error_dual

    def spy_filter(ctx, half_a, half_b, rects, counts_a, counts_b, out_fb, err_img=None, **kw):
        calls.append(("filter", list(rects), dict(kw)))
        return real_filter(ctx, half_a, half_b, rects, counts_a, counts_b, out_fb, err_img, **kw)

    def spy_error(ctx, err_img, rects):
        errors = real_error(ctx, err_img, rects)
        calls.append(("error", list(rects), [float(e) for e in errors]))
        return errors

    monkeypatch.setattr(render, "denoise_atrous_dual", spy_filter)
    monkeypatch.setattr(render, "tile_error_dual", spy_error)

    def settings(**kw):
        return Settings(scenes.camera(HW, HH), samples_per_iteration=2, denoise_dual=True, denoise_dual_atrous=True, denoise_dual_features=True, adaptive_min_samples=4,
                        **HCOMMON, **kw)

    render.render_tiled(sc, settings(adaptive_denoised_threshold=1e-300), devices=(0,))
    threshold = float(np.median(calls[1][2]))
    del calls[:]
    off = render.render_tiled(sc, settings(adaptive_denoised_threshold=threshold), devices=(0,))
    calls_off = list(calls)
    del calls[:]
    on = render.render_tiled(sc, settings(adaptive_denoised_threshold=threshold, denoise_dual_atrous_region=True), devices=(0,))
    calls_on = list(calls)
    del calls[:]
    filters_on, filters_off = [c for c in calls_on if c[0] == "filter"], [c for c in calls_off if c[0] == "filter"]
    assert len(filters_on) == len(filters_off) >= 2
    assert all(c[2]["slope"] == 3.0 and "region" in c[2] for c in filters_on) and all(c[2]["slope"] == 3.0 and "region" not in c[2] for c in filters_off)
    live = [c[1] for c in calls_on if c[0] == "error"]
    assert live[0] == tiles and 0 < len(live[1]) < len(tiles)
    assert [np.float64(c[2]).tobytes() for c in calls_on if c[0] == "error"] == [np.float64(c[2]).tobytes() for c in calls_off if c[0] == "error"]
    got, expected = [_message_key(m) for m in on._messages], [_message_key(m) for m in off._messages]
    assert len(got) == len(expected) and all(g == e for g, e in zip(got, expected))
    fin = tgd._finished_tiles(on)
    assert min(t.sample_count for t in fin) < HSPP  # some tiles finished early
    off.async_await()  # (past the progress snapshots, as await_ needs them)
    frame_on, frame_off = on.await_(), off.await_()
    assert frame_on.tobytes() == frame_off.tobytes() and np.isfinite(frame_on).all()
    monkeypatch.undo()
    halves, rects, counts_a, counts_b = _assemble_dual(fin, HW, HH)
    counts_f = [a + b for a, b in zip(counts_a, counts_b)]
    ds = render.DeviceScene(gpu_ctx, sc)
    try:
        F, G = _direct_features(gpu_ctx, ds, Settings(scenes.camera(HW, HH), sample_count=HSPP, bounce_limit=HBOUNCES, seed=scenes.SEED), rects, counts_f)
    finally:
        ds.close()
    guide = dict(features=F, features_sq=G, counts_f=counts_f, **HGUIDE)
    direct, _ = render.denoise_atrous_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, slope=3.0, **HFILTER, **guide)
    assert frame_on.tobytes() == direct.tobytes()
    assert direct.tobytes() != render.denoise_atrous_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, **HFILTER, **guide)[0].tobytes()  # the slope mattered
    extra = ["--spi", "2", "--denoise-dual", "1", "--denoise-dual-atrous", "1", "--denoise-dual-features", "1", "--adaptive-denoised", "%.17g" % threshold, "--adaptive-min", "4"]
    assert _run_cli(tmp_path, "off", extra).tobytes() == frame_on.tobytes()
    assert _run_cli(tmp_path, "on", extra + ["--denoise-dual-atrous-region", "1"]).tobytes() == frame_on.tobytes()


# ---------------------------------------------------------------- quality on real renders
@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_quality_at_16_spp_at_the_shipped_values(gpu_ctx, which):
    """256 x 144, 16 spp against 2,048 spp of seed + 1, the shipped levels, k, alpha, k_f, tau and slope 3, against rmd_denoise_atrous guided on the same
    sums (test_gpu_denoise_atrous.test_quality_at_16_spp_at_the_defaults' frames).  Computed first on the CPU at this size (tools/atrous_slope_bars.py:
    the restatement, the oracle's per-sample frames, first_hit_ref.first_hit_sums):
        ReflectiveSpheres  unfiltered 0.10679, unguided 0.02342, guided 0.02212, slope 2 0.02193, slope 3 0.02169 (x0.9805), slope 5 0.02161 (x0.9767)
        mesh stand-in      unfiltered 0.10642, unguided 0.02817, guided 0.02706, slope 2 0.02754, slope 3 0.02750 (x1.0164), slope 5 0.02732 (x1.0096)
    The spheres ratio at this size, x0.9805, is above 0.98 — thinner than the x0.932 seen at 128 x 72 —, so by the rule set before the figures were known
    the test asserts on both scenes only that the sloped frame beats the unfiltered mean, and prints the ratios.  On the mesh at this size the term costs
    1.6 %."""
    W, H = 256, 144
    sc = scenes.reflective_spheres() if which == "spheres" else scenes.gold_dragon_standin(n=24)
    S_ref, _ = tgd.render_moments(gpu_ctx, sc, W, H, 2048, seed=scenes.SEED + 1)
    ref = S_ref / 2048.0
    S, Q = tgd.render_moments(gpu_ctx, sc, W, H, 16, seed=scenes.SEED)
    F, G = tgg._feature_sums(gpu_ctx, sc, W, H, 16, scenes.SEED)
    rect, count = [(0, 0, W, H)], [16]
    st = Settings(scenes.camera(W, H), 16)  # the shipped defaults
    params = dict(levels=st.denoise_atrous_levels, k=st.denoise_atrous_k, alpha=st.denoise_alpha, k_f=st.denoise_feature_k, tau=st.denoise_feature_tau)
    noisy = tgd.rmse(S / 16.0, ref)
    gd = tgd.rmse(render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, rect, count, **params), ref)
    sl = tgd.rmse(render.denoise_atrous_arrays(gpu_ctx, S, Q, F, G, rect, count, slope=3.0, **params), ref)
    print("atrous slope quality: %s 256x144 16 spp: RMSE unfiltered %.5g, guided %.5g, slope 3 %.5g = x%.4f of guided" % (which, noisy, gd, sl, sl / gd))
    assert sl < noisy, (sl, noisy)
