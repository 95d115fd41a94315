"""The denoise kernels against their restatements on adversarial frames (tests/denoise_frames.py): every window (r, f) the header allows, frames at the
tile edges, invalid pixels on the kernels' seams, scales from 2^-500 to 2^500, and region sets along the seams.

The bar is denoise_frames.agree: test_gpu_denoise._agree's 1e-9 relative and its NaN and infinity rules, with the absolute allowance taken from the
output pixel's own window (1e-12 of the largest |u| the pixel can be a mean of) instead of from the whole frame; err of the
non-local-means dual calls is held to the same bar with 1e-12 of that scale squared.  Beyond agreement the header's exact
promises: a pixel that is not valid comes back as S / n bit for bit, err is NaN exactly at the pixels that are not dual-valid, inputs are untouched.
Every test prints the worst relative difference it saw ("FRAMES ..." lines; DESIGN.md section 26 records them)."""
import numpy as np
import pytest

import denoise_atrous_dual_ref as adref
import denoise_atrous_ref as aref
import denoise_dual_guided_ref as dgref
import denoise_dual_ref
import denoise_dual_select_ref as sref
import denoise_frames as df
import denoise_guided_ref as gref
import denoise_ref
import denoise_slope_ref as slref
from denoise_ref import mean_and_variance
from raymond_amd import probe, render
from test_gpu_denoise import _agree
from test_gpu_denoise_dual import _two_halves
from test_gpu_denoise_dual_region import _bits, _expect, _mask, _random_bytes
from test_gpu_denoise_dual_select import WINDOWS, _Select, _cands, _inputs_with_a_noise_floor

pytestmark = pytest.mark.gpu

K, ALPHA = 0.45, 1.0
GUIDE = dict(k_f=1.0, tau=1e-2)  # the shipped guide: on denoise_frames' features the feature weight cuts most weights and isolates few pixels
RIM_GUIDE = dict(k_f=0.6, tau=1e-3)  # the sharper one, on the window grid's rim
SLOPE = 3.0
ALL_R, ALL_F = tuple(range(13)), tuple(range(5))
RIM = sorted({(r, f) for r in (0, 1, 11, 12) for f in ALL_F} | {(r, 4) for r in ALL_R} | {(12, 3)})
SELECT_WINDOWS = ((12, 3), (11, 4), (12, 4), (1, 4))
SHAPE_WINDOWS = ((3, 1), (12, 3), (12, 4))  # a small window and the largest layout of each tile width
WINDOWS_2 = ((3, 1), (12, 4))
GRID_FRAME = (49, 33)


def _note(entry, cls, window, worst):
    """worst: (the worst relative difference, |ref| / scale where it lies) as denoise_frames.agree returns them, or the difference alone."""
    worst, share = worst if isinstance(worst, tuple) else (worst, float("nan"))
    print("FRAMES entry=%s class=%s window=%s worst=%.3g share=%.3g" % (entry, cls, "%d,%d" % window if isinstance(window, tuple) else window, worst, share))


class _Dev:
    """One frame on the device: the halves and both feature pairs uploaded once, out and err re-filled with random bytes before every call (a pixel
    the kernel does not write cannot pass)."""

    def __init__(self, ctx, halves, rects, counts_a, counts_b, counts_f, F, G, F1, G1, guide, seed=1):
        self.ctx, self.rng, self.guide = ctx, np.random.default_rng(seed), guide
        self.rects, self.counts = rects, (counts_a, counts_b, counts_f)
        self.H, self.W = halves[0].shape[:2]
        self.host = list(halves) + [F, G, F1, G1]
        self.fbs = [render.Framebuffer(ctx, self.W, self.H) for _ in range(5)]
        self.err = render.ErrorImage(ctx, self.W, self.H)
        self.feat = [render.FeatureBuffer(ctx, self.W, self.H) for _ in range(4)]
        for buf, arr in zip(self.fbs[:4] + self.feat, self.host):
            buf.upload(arr)

    def _fill(self):
        self.out_init, self.err_init = _random_bytes(self.rng, (self.H, self.W, 3)), _random_bytes(self.rng, (self.H, self.W))
        self.fbs[4].upload(self.out_init), self.err.upload(self.err_init)

    def single(self, guided=False, slope=None, **params):
        self._fill()
        if guided:
            render.denoise_guided(self.ctx, self.fbs[0], self.fbs[1], self.feat[2], self.feat[3], self.rects, self.counts[0], self.fbs[4], slope=slope, **self.guide, **params)
        else:
            render.denoise(self.ctx, self.fbs[0], self.fbs[1], self.rects, self.counts[0], self.fbs[4], **params)
        return self.fbs[4].download()

    def dual(self, guided=False, slope=None, region=None, **params):
        self._fill()
        kw = dict(features=self.feat[0], features_sq=self.feat[1], counts_f=self.counts[2], slope=slope, **self.guide) if guided else {}
        render.denoise_dual(self.ctx, (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3]), self.rects, self.counts[0], self.counts[1], self.fbs[4], self.err,
                            region=region, **kw, **params)
        return self.fbs[4].download(), self.err.download()

    def atrous(self, guided, levels):
        self._fill()
        kw = dict(features=self.feat[2], features_sq=self.feat[3], **self.guide) if guided else {}
        render.denoise_atrous(self.ctx, self.fbs[0], self.fbs[1], self.rects, self.counts[0], self.fbs[4], levels=levels, **kw)
        return self.fbs[4].download()

    def atrous_dual(self, guided, levels):
        self._fill()
        kw = dict(features=self.feat[0], features_sq=self.feat[1], counts_f=self.counts[2], **self.guide) if guided else {}
        render.denoise_atrous_dual(self.ctx, (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3]), self.rects, self.counts[0], self.counts[1], self.fbs[4], self.err,
                                   levels=levels, **kw)
        return self.fbs[4].download(), self.err.download()

    def assert_inputs_untouched(self, what):
        for buf, arr in zip(self.fbs[:4] + self.feat, self.host):
            assert buf.download().tobytes() == np.ascontiguousarray(arr, dtype=np.float64).tobytes(), "%s: an input buffer changed" % what

    def close(self):
        for b in self.fbs + [self.err] + self.feat:
            b.close()


class _Case:
    """A frame with what the checks need of it, and its _Dev."""

    def __init__(self, ctx, name, halves, rects, counts_a, counts_b, counts_f, n_a, n_b, n_f, F, G, F1, G1, k=K, alpha=ALPHA, guide=GUIDE):
        self.name, self.halves, self.n_a, self.n_b, self.n_f, self.F, self.G, self.F1, self.G1, self.k, self.alpha = name, halves, n_a, n_b, n_f, F, G, F1, G1, k, alpha
        self.guide = dict(guide)
        self.u_a, self.v_a, self.ok_a = mean_and_variance(halves[0], halves[1], n_a)
        self.u_b, self.v_b, self.ok_b = mean_and_variance(halves[2], halves[3], n_b)
        self.dual_valid = self.ok_a & self.ok_b
        with np.errstate(all="ignore"):
            self.raw = halves[0] / n_a.astype(np.float64)[..., None]
            self.merged = (halves[0] + halves[2]) / (n_a.astype(np.float64) + n_b.astype(np.float64))[..., None]
        self.dev = _Dev(ctx, halves, rects, counts_a, counts_b, counts_f, F, G, F1, G1, self.guide)

    @staticmethod
    def of(ctx, name):
        fr = df.frame(name)
        F1, G1 = fr.single_features()
        return _Case(ctx, name, fr.halves, fr.rects, fr.counts_a, fr.counts_b, fr.counts_f, fr.n_a, fr.n_b, fr.n_f, fr.F, fr.G, F1, G1, fr.k, fr.alpha)

    # ---- the single-buffer calls
    def check_single(self, window, guided=False, slope=None):
        r, f = window
        entry = "rmd_denoise" + ("_guided" if guided else "") + ("_slope" if slope is not None else "")
        params = dict(radius=r, patch_radius=f, k=self.k, alpha=self.alpha)
        out = self.dev.single(guided, slope, **params)
        S, Q = self.halves[:2]
        if not guided:
            ref = denoise_ref.denoise(S, Q, self.n_a, **params)
        elif slope is None:
            ref = gref.denoise_guided(S, Q, self.F1, self.G1, self.n_a, **params, **self.guide)
        else:
            ref = slref.denoise_guided_slope(S, Q, self.F1, self.G1, self.n_a, **params, **self.guide, slope=slope)
        what = "%s on %s at (%d, %d)" % (entry, self.name, r, f)
        worst = df.agree(out, ref, df.local_scale([self.u_a], self.ok_a, r), what)
        assert out[~self.ok_a].tobytes() == self.raw[~self.ok_a].tobytes(), "%s: a pixel that is not valid is not S / n" % what
        _note(entry, self.name, window, worst)
        return out

    # ---- the dual calls
    def ref_dual(self, window, guided=False, slope=None):
        """-> f_A, f_B, out, err of the restatement (denoise_dual_guided_ref.filtered_halves' operations; with a slope, denoise_slope_ref's denominator)."""
        r, f = window
        guide = None
        if guided:
            guide = dgref.feature_planes(self.F, self.G, self.n_f, self.dual_valid, **self.guide) if slope is None else \
                slref._dual_guide(self.F, self.G, self.n_f, self.dual_valid, self.guide["k_f"], self.guide["tau"], slope)
        f_a = dgref.cross_filter(self.u_b, self.v_b, self.u_a, self.dual_valid, r, f, self.k, self.alpha, guide)
        f_b = dgref.cross_filter(self.u_a, self.v_a, self.u_b, self.dual_valid, r, f, self.k, self.alpha, guide)
        out, err = denoise_dual_ref.combine(f_a, f_b, self.halves[0], self.halves[2], self.n_a, self.n_b, self.dual_valid)
        return f_a, f_b, out, err

    def check_dual_result(self, entry, window, reach, out, err, f_a, f_b, out_ref, err_ref=None):
        """err_ref given (the non-local-means calls): err is held to it at the frame's own bar, 1e-9 relative with 1e-12 of the local scale of err;
        without it (the a-trous pair): to the filtered halves by the reasoning of the a-trous dual file."""
        what = "%s on %s at %s" % (entry, self.name, window)
        scale = df.local_scale([self.u_a, self.u_b], self.dual_valid, reach)
        worst = df.agree(out, out_ref, scale, what)
        if err_ref is None:
            worst_err = df.agree_err_propagated(err, f_a, f_b, self.dual_valid, scale, what)
        else:
            worst_err = df.agree_err(err, err_ref, self.dual_valid, scale, what)
        assert out[~self.dual_valid].tobytes() == self.merged[~self.dual_valid].tobytes(), "%s: a pixel that is not dual-valid is not (S_a + S_b) / (n_a + n_b)" % what
        assert np.array_equal(np.isnan(err), ~self.dual_valid), "%s: NaN in err elsewhere than at the pixels that are not dual-valid" % what
        _note(entry, self.name, window, worst)
        _note(entry + ":err", self.name, window, worst_err)

    def check_dual(self, window, guided=False, slope=None):
        entry = "rmd_denoise_dual" + ("_guided" if guided else "") + ("_slope" if slope is not None else "")
        out, err = self.dev.dual(guided, slope, radius=window[0], patch_radius=window[1], k=self.k, alpha=self.alpha)
        f_a, f_b, out_ref, err_ref = self.ref_dual(window, guided, slope)
        self.check_dual_result(entry, window, window[0], out, err, f_a, f_b, out_ref, err_ref)
        return out, err

    # ---- the a-trous pair
    def check_atrous(self, level_counts):
        S, Q = self.halves[:2]
        for guided in (False, True):
            refs = aref.atrous_all(S, Q, self.n_a, level_counts, **(dict(F=self.F1, G=self.G1, **self.guide) if guided else {}))
            drefs, dual = adref.filtered_halves_all(*self.halves, self.n_a, self.n_b, level_counts, **(dict(F=self.F, G=self.G, n_f=self.n_f, **self.guide) if guided else {}))
            assert np.array_equal(dual, self.dual_valid)
            for levels in level_counts:
                reach = 2 * ((1 << levels) - 1)
                window = "%d levels%s" % (levels, ", guided" if guided else "")
                what = "rmd_denoise_atrous on %s at %s" % (self.name, window)
                out = self.dev.atrous(guided, levels)
                worst = df.agree(out, refs[levels], df.local_scale([self.u_a], self.ok_a, reach), what)
                assert out[~self.ok_a].tobytes() == self.raw[~self.ok_a].tobytes(), "%s: a pixel that is not valid is not S / n" % what
                _note("rmd_denoise_atrous", self.name, window, worst)
                out, err = self.dev.atrous_dual(guided, levels)
                f_a, f_b = drefs[levels]
                out_ref, _ = denoise_dual_ref.combine(f_a, f_b, self.halves[0], self.halves[2], self.n_a, self.n_b, dual)
                self.check_dual_result("rmd_denoise_atrous_dual", window, reach, out, err, f_a, f_b, out_ref)


@pytest.fixture(scope="module")
def cases(gpu_ctx):
    """name -> _Case, made on first use and closed when the module is done (the frames are a few thousand pixels each)."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Case.of(gpu_ctx, name)
        return made[name]

    yield get
    for c in made.values():
        c.dev.close()


# ---------------------------------------------------------------- 1. the whole window grid
@pytest.fixture(scope="module")
def grid(gpu_ctx):
    """One 49 x 33 frame in test_gpu_denoise_dual._two_halves' style: 8 x 16 tiles with unequal counts in the halves (a 0 and a 1 in each), one tile
    uncovered, poisoned sums; denoise_frames' features at counts of their own (a 0 and a 1 among them) with a NaN in F and an infinite G at a few pixels, and at
    half A's counts for the single-buffer calls."""
    W, H = GRID_FRAME
    rng = np.random.default_rng(W * 1000 + H + 31)
    halves, rects, counts_a, counts_b, n_a, n_b = _two_halves(rng, W, H)
    counts_f = [int(c) for c in rng.integers(2, 100, len(rects))]
    counts_f[6], counts_f[7] = 0, 1
    n_f = denoise_ref.count_image(W, H, rects, counts_f)
    means = df.feature_means(rng, W, H)
    f_nan, g_inf = rng.uniform(size=(H, W)) < 0.01, rng.uniform(size=(H, W)) < 0.01
    F, G = df.feature_sums(*means, n_f, f_nan, g_inf)
    F1, G1 = df.feature_sums(*means, n_a, f_nan, g_inf)
    case = _Case(gpu_ctx, "grid_49x33", halves, rects, counts_a, counts_b, counts_f, n_a, n_b, n_f, F, G, F1, G1, guide=RIM_GUIDE)
    assert case.dual_valid.any() and not case.ok_a.all() and not case.ok_b.all()
    yield case
    case.dev.assert_inputs_untouched("the window grid")
    case.dev.close()


@pytest.mark.parametrize("f", ALL_F, ids=lambda f: "f%d" % f)
@pytest.mark.parametrize("r", ALL_R, ids=lambda r: "r%d" % r)
def test_every_window_single_and_dual(grid, r, f):
    """All 13 x 5 windows of rmd_denoise and rmd_denoise_dual: every LDS layout the launchers can make, at either tile width."""
    tw, lds, _, budget = probe.denoise_tile(r, f)
    assert lds <= budget and tw == (24 if (r, f) == (12, 4) else 32)
    out = grid.check_single((r, f))
    grid.check_dual((r, f))
    if r == 0:  # the mean bit for bit
        assert out.tobytes() == grid.raw.tobytes()


@pytest.mark.parametrize("r,f", RIM, ids=lambda v: str(v))
def test_the_rim_of_the_window_grid_guided_and_with_the_slope(grid, r, f):
    for slope in (None, SLOPE):
        grid.check_single((r, f), guided=True, slope=slope)
        grid.check_dual((r, f), guided=True, slope=slope)


@pytest.mark.parametrize("r,f", SELECT_WINDOWS)
def test_select_at_the_largest_layouts(gpu_ctx, r, f):
    """test_gpu_denoise_dual_select.test_select_matches_the_restatement_stage_by_stage's comparison and its near-tie rule, unchanged, on its own kind of frame
    (a noise floor, so that near ties are rare) at 49 x 33 and at the windows whose LDS layouts are the largest; windows (2, 2) of its WINDOWS."""
    W, H = GRID_FRAME
    halves, rects, counts_a, counts_b, n_a, n_b, F, G, counts_f, n_f = _inputs_with_a_noise_floor(W, H)
    cands = _cands(K, ALPHA)[:3]
    sw, lw = WINDOWS[2]
    kw = dict(radius=r, patch_radius=f, sure_window=sw, select_window=lw)
    bufs = _Select(gpu_ctx, halves, F, G)
    try:
        bufs.fill(np.random.default_rng(r * 10 + f))
        dev = bufs.run(rects, counts_a, counts_b, counts_f, cands, **kw)
    finally:
        bufs.close()
    planes = sref._planes(*halves, n_a, n_b)
    parts = [sref.candidate(planes, n_a, n_b, c, F, G, n_f, r, f) for c in cands]
    own = sref.denoise_dual_select(*halves, n_a, n_b, cands, F, G, n_f, parts=parts, **kw)
    dual = own["dual"]
    assert np.array_equal(dev["win"] == sref.NO_WINNER, ~dual)
    tie = sref.near_ties(own["E"], dual)
    print("select %dx%d r %d f %d: %d near ties of %d dual-valid pixels, %d winners differ" % (W, H, r, f, tie.sum(), dual.sum(), (dev["win"] != own["own_win"]).sum()))
    assert tie.sum() <= 0.01 * dual.sum()
    assert np.array_equal(dev["win"][~tie], own["own_win"][~tie])
    ref = sref.denoise_dual_select(*halves, n_a, n_b, cands, F, G, n_f, parts=parts, win=dev["win"], **kw)
    u_a, u_b = planes[0], planes[2]
    worst = df.agree(dev["out"], ref["out"], df.local_scale([u_a, u_b], dual, r + lw), "rmd_denoise_dual_select at (%d, %d)" % (r, f))
    _note("rmd_denoise_dual_select", "grid_49x33_noise_floor", (r, f), worst)
    for name in ("err", "sure"):  # (not means of u: test_gpu_denoise's bar, as there)
        _agree(dev[name], ref[name])


# ---------------------------------------------------------------- 2. shapes
@pytest.mark.parametrize("window", SHAPE_WINDOWS, ids=lambda w: "r%d_f%d" % w)
@pytest.mark.parametrize("name", df.names("shape_"))
def test_shapes_at_the_tile_edges(cases, name, window):
    case = cases(name)
    case.check_single(window)
    case.check_dual(window)
    case.check_dual(window, guided=True)
    case.dev.assert_inputs_untouched(name)


@pytest.mark.parametrize("name", df.names("shape_"))
def test_shapes_through_the_atrous_pair(cases, name):
    cases(name).check_atrous((1, aref.MAX_LEVELS))


# ---------------------------------------------------------------- 3. seams and scales
@pytest.mark.parametrize("window", WINDOWS_2, ids=lambda w: "r%d_f%d" % w)
@pytest.mark.parametrize("name", df.names("seam_") + df.names("scale_"))
def test_seams_and_scales(cases, name, window):
    case = cases(name)
    out = case.check_single(window)
    case.check_single(window, guided=True)
    dual_out, err = case.check_dual(window)
    case.check_dual(window, guided=True)
    case.dev.assert_inputs_untouched(name)
    if name.startswith("seam_all_"):  # the all-invalid frame is S / n everywhere
        if name != "seam_all_b" and name != "seam_all_f":
            assert not case.ok_a.any() and out.tobytes() == case.raw.tobytes(), name
        if name != "seam_all_f":
            assert not case.dual_valid.any() and dual_out.tobytes() == case.merged.tobytes() and np.isnan(err).all(), name
    if name == "seam_ring_a" and window[0] <= df.RING_DEPTH:  # nothing else is valid within the window: out = (1 * u) / 1
        y, x = df.RING_PIXEL
        assert case.ok_a[y, x] and out[y, x].tobytes() == case.u_a[y, x].tobytes(), name
    if name == "scale_flat":  # every weight is 1 and every sum of 0.75s is exact
        assert out.tobytes() == case.u_a.tobytes() and dual_out.tobytes() == case.u_a.tobytes() and (err == 0.0).all(), name
    if name == "scale_overflow":  # NaN distances became weights of 1, not NaN pixels
        assert np.isfinite(out).all() and np.isfinite(dual_out).all() and np.isfinite(err).all(), name


@pytest.mark.parametrize("name", df.names("seam_") + df.names("scale_"))
def test_seams_and_scales_through_the_atrous_pair(cases, name):
    cases(name).check_atrous((3,))


# ---------------------------------------------------------------- 4. regions
REGION_FRAME = "seam_ring_ab"  # 640 of 800 pixels dual-valid on both sides of every seam; each half's ring gives rects of invalid pixels and crosses the seam columns
REGION_CALLS = {"rmd_denoise_dual_region": dict(), "rmd_denoise_dual_guided_region": dict(guided=True), "rmd_denoise_dual_guided_slope_region": dict(guided=True, slope=SLOPE)}


@pytest.mark.parametrize("call", list(REGION_CALLS))
@pytest.mark.parametrize("window", ((12, 3), (12, 4)), ids=lambda w: "r%d_f%d" % w)
def test_regions_along_the_seams(cases, window, call):
    """The whole-frame call agrees with the restatement; inside the region its bytes, everywhere else the random bytes the buffers held."""
    case = cases(REGION_FRAME)
    dev, W, H = case.dev, case.dev.W, case.dev.H
    params = dict(radius=window[0], patch_radius=window[1], k=case.k, alpha=case.alpha, **REGION_CALLS[call])
    full_out, full_err = case.check_dual(window, **REGION_CALLS[call])
    assert np.isnan(full_err).any() and np.isfinite(full_err).any()
    sets = df.region_sets(W, H, ~case.dual_valid)
    assert len(sets) == 7
    for name, region in sets.items():
        mask = _mask(W, H, region)
        out, err = dev.dual(region=region, **params)
        assert _bits(out).tobytes() == _expect(mask, full_out, dev.out_init).tobytes(), (call, name, window)
        assert _bits(err).tobytes() == _expect(mask, full_err, dev.err_init).tobytes(), (call, name, window)
    dev.assert_inputs_untouched(call)
