"""rmd_denoise_dual_select on the device: every stage against the numpy restatement (tests/denoise_dual_select_ref.py), the definition's exact
consequences (one candidate is the existing call, a duplicated candidate changes nothing, window 0 hands out one candidate's own pixels, radius 0
is the closed form, NULL outputs leave the others alone), the host paths (Python render_tiled / await_, the C++ mirror through raymond_cli), and on
rendered frames the quality of the selected frame and the calibration of SURE against the true error.

The frames, counts, poison and tolerance are test_gpu_denoise_dual_guided.py's own (imported from it and from the files it imports from)."""
import os
import subprocess

import numpy as np
import pytest

import denoise_dual_select_ref as sref
import denoise_ref
from raymond_amd import render, scenes
from raymond_amd.scene import Settings, generate_tiles
from test_gpu_denoise import CASES, _agree, _finished_tiles, _poison, _tiles_with_counts
from test_gpu_denoise_dual import CLI, _assemble_dual, _cli, _two_halves
from test_gpu_denoise_dual_guided import (HBOUNCES, HH, HSPI, HSPP, HW, _direct_features, _direct_halves, _features, _inputs, _scene, _settings)
from test_gpu_denoise_dual_region import _message_key, _random_bytes

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 200), (37, 23), (64, 48)]
WINDOWS = [(0, 0), (1, 2), (2, 2)]


def _cands(k, alpha):
    """Four candidates around a CASES row: the row's own unguided filter, a guided one at k = 1.0, an unguided one at a larger k, a guided one at a smaller k
    with the sharper guide.  (The test against the restatement takes the first two or three: test_gpu_denoise_dual_guided.py's features are random per
    pixel, so two GUIDED candidates both leave most pixels alone with themselves and tie there to within rounding.)"""
    return [dict(k=k, alpha=alpha), dict(k=1.0, alpha=alpha, guided=True, k_f=1.0, tau=1e-2), dict(k=1.6 * k, alpha=alpha),
            dict(k=0.7 * k, alpha=alpha, guided=True, k_f=0.6, tau=1e-3)]


def _moments_with_a_noise_floor(rng, n_img):
    """test_gpu_denoise.py's _moments with the noise level drawn from [0.3, 0.6] instead of [0, 0.6] and the variance factor from [0.5, 1.5] instead of
    [0, 1].  A pixel whose variance is next to nothing is further than exp can tell from every neighbour; every candidate then returns u there, and
    their SUREs differ by rounding alone: near ties, on which no argmin can be held to another."""
    H, W = n_img.shape
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([0.5 + 0.4 * np.sin(x / 5.0), 0.3 + 0.2 * np.cos(y / 3.0), 0.2 + 0.1 * ((x + y) % 7)], axis=-1)
    sigma = rng.uniform(0.3, 0.6, (H, W, 1)) * (1 + (x % 9 == 0))[..., None]
    n = np.maximum(n_img, 0).astype(np.float64)[..., None]
    mean = base + rng.normal(0.0, 1.0, (H, W, 3)) * sigma / np.sqrt(np.maximum(n, 1.0))
    S = mean * n
    Q = S * mean + rng.uniform(0.5, 1.5, (H, W, 3)) * sigma * sigma * np.maximum(n - 1.0, 0.0)
    Q[rng.uniform(size=(H, W, 3)) < 0.02] *= 0.5  # some below S^2 / n: a negative variance estimate, clamped to 0
    return S, Q


def _inputs_with_a_noise_floor(W, H):
    """_inputs' frame — the same tiling, unequal counts with 0 and 1 in each half, one tile uncovered, the same poison, the same features — over
    _moments_with_a_noise_floor.  The seed was chosen on the CPU: over every case, candidate count and window pair of the test below the restatement has
    at most 1 near tie per frame (0.25 % of the dual-valid pixels, a quarter of the cap); _inputs itself gives up to 23 %."""
    rng = np.random.default_rng(W * 1000 + H + 23)
    rects, counts_a = _tiles_with_counts(W, H, 8, 16, rng) if W * H > 1 else ([(0, 0, 1, 1)], [9])
    counts_b = [int(c) for c in rng.integers(2, 65, len(rects))] if W * H > 1 else [5]
    if len(rects) >= 6:
        counts_b[4], counts_b[5] = 0, 1
    n_a, n_b = denoise_ref.count_image(W, H, rects, counts_a), denoise_ref.count_image(W, H, rects, counts_b)
    S_a, Q_a = _moments_with_a_noise_floor(rng, n_a)
    S_b, Q_b = _moments_with_a_noise_floor(rng, n_b)
    if W * H > 1:
        _poison(S_a, Q_a, rng)
        _poison(S_b, Q_b, rng)
    F, G, counts_f, n_f = _features(rng, W, H, rects)
    return (S_a, Q_a, S_b, Q_b), rects, counts_a, counts_b, n_a, n_b, F, G, counts_f, n_f


class _Select:
    """The two halves and the features uploaded once; the four outputs re-filled before each call."""

    def __init__(self, ctx, halves, F, G):
        self.ctx = ctx
        H, W = halves[0].shape[:2]
        self.shape = (H, W)
        self.fbs = [render.Framebuffer(ctx, W, H) for _ in range(5)]
        self.err, self.sure, self.win = render.ErrorImage(ctx, W, H), render.ErrorImage(ctx, W, H), render.WinnerImage(ctx, W, H)
        self.feat = [render.FeatureBuffer(ctx, W, H), render.FeatureBuffer(ctx, W, H)]
        for fb, arr in zip(self.fbs, halves):
            fb.upload(arr)
        self.feat[0].upload(F), self.feat[1].upload(G)

    def fill(self, rng):
        """Random bytes into the four outputs -> what they hold."""
        H, W = self.shape
        init = dict(out=_random_bytes(rng, (H, W, 3)), err=_random_bytes(rng, (H, W)), sure=_random_bytes(rng, (H, W)),
                    win=rng.integers(0, 2**32, (H, W), dtype=np.uint64).astype(np.uint32))
        self.fbs[4].upload(init["out"]), self.err.upload(init["err"]), self.sure.upload(init["sure"]), self.win.upload(init["win"])
        return init

    def run(self, rects, counts_a, counts_b, counts_f, cands, want=("err", "sure", "win"), **params):
        imgs = dict(err=self.err, sure=self.sure, win=self.win)
        render.denoise_dual_select(self.ctx, (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3]), rects, counts_a, counts_b, cands, self.fbs[4],
                                   *(imgs[n] if n in want else None for n in ("err", "sure", "win")), features=self.feat[0], features_sq=self.feat[1],
                                   counts_f=counts_f, **params)
        return dict(out=self.fbs[4].download(), err=self.err.download(), sure=self.sure.download(), win=self.win.download())

    def plain(self, rects, counts_a, counts_b, counts_f, cand, radius, patch_radius):
        """The existing call of one candidate: rmd_denoise_dual, or rmd_denoise_dual_guided -> out, err"""
        k, alpha, guided, k_f, tau = sref._cand(cand)
        kw = dict(features=self.feat[0], features_sq=self.feat[1], counts_f=counts_f, k_f=k_f, tau=tau) if guided else {}
        render.denoise_dual(self.ctx, (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3]), rects, counts_a, counts_b, self.fbs[4], self.err, radius=radius,
                            patch_radius=patch_radius, k=k, alpha=alpha, **kw)
        return self.fbs[4].download(), self.err.download()

    def close(self):
        for b in self.fbs + [self.err, self.sure, self.win] + self.feat:
            b.close()


# ---------------------------------------------------------------- 1. stage by stage against the restatement
@pytest.mark.parametrize("W,H", SHAPES)
def test_select_matches_the_restatement_stage_by_stage(gpu_ctx, W, H):
    """out, err and sure against the restatement RUN ON THE DEVICE'S WINNERS (the device's exp may flip an argmin at a near tie; after the winners
    everything is exact arithmetic on agreed inputs), and the device's winners against the restatement's own everywhere but at its near ties: two
    smallest window means within 1e-9 * max|E| of each other and not equal — at most 1 % of the dual-valid pixels (_inputs_with_a_noise_floor)."""
    halves, rects, counts_a, counts_b, n_a, n_b, F, G, counts_f, n_f = _inputs_with_a_noise_floor(W, H)
    bufs = _Select(gpu_ctx, halves, F, G)
    try:
        for r, f, k, alpha in CASES:
            cands = _cands(k, alpha)[:3]
            planes = sref._planes(*halves, n_a, n_b)
            parts = [sref.candidate(planes, n_a, n_b, c, F, G, n_f, r, f) for c in cands]
            for n in (2, 3):
                for sw, lw in WINDOWS:
                    kw = dict(radius=r, patch_radius=f, sure_window=sw, select_window=lw)
                    dev = bufs.run(rects, counts_a, counts_b, counts_f, cands[:n], **kw)
                    own = sref.denoise_dual_select(*halves, n_a, n_b, cands[:n], F, G, n_f, parts=parts[:n], **kw)
                    dual = own["dual"]
                    assert np.array_equal(dev["win"] == sref.NO_WINNER, ~dual)
                    tie = sref.near_ties(own["E"], dual)
                    print("select %dx%d r %d f %d k %g alpha %g, %d candidates, windows %d %d: %d near ties of %d dual-valid pixels, %d winners differ" %
                          (W, H, r, f, k, alpha, n, sw, lw, tie.sum(), dual.sum(), (dev["win"] != own["own_win"]).sum()))
                    assert tie.sum() <= 0.01 * dual.sum()
                    assert np.array_equal(dev["win"][~tie], own["own_win"][~tie])
                    ref = sref.denoise_dual_select(*halves, n_a, n_b, cands[:n], F, G, n_f, parts=parts[:n], win=dev["win"], **kw)
                    for name in ("out", "err", "sure"):
                        _agree(dev[name], ref[name])  # (NaN exactly where the restatement has NaN)
            if r == 3 and W * H > 100:  # more than one candidate wins somewhere
                assert len(set(own["own_win"][dual].tolist())) >= 2
    finally:
        bufs.close()


# ---------------------------------------------------------------- 2. one candidate is the existing call
@pytest.mark.parametrize("W,H", SHAPES)
def test_one_candidate_is_the_existing_call_bit_for_bit(gpu_ctx, W, H):
    rng, halves, rects, counts_a, counts_b, _, _, F, G, counts_f, _ = _inputs(W, H)
    bufs = _Select(gpu_ctx, halves, F, G)
    try:
        for r, f, k, alpha in CASES:
            for cand in _cands(k, alpha)[:2]:  # unguided: rmd_denoise_dual; guided: rmd_denoise_dual_guided
                for sw, lw in ((0, 0), (2, 2)):
                    bufs.fill(rng)
                    got = bufs.run(rects, counts_a, counts_b, counts_f, [cand], radius=r, patch_radius=f, sure_window=sw, select_window=lw)
                    out, err = bufs.plain(rects, counts_a, counts_b, counts_f, cand, r, f)
                    assert got["out"].tobytes() == out.tobytes() and got["err"].tobytes() == err.tobytes(), (r, f, cand)
                    assert np.array_equal(got["win"] == 0, ~np.isnan(err)) and np.all(got["win"][np.isnan(err)] == sref.NO_WINNER)
        if W * H > 1:
            assert np.isnan(err).any() and np.isfinite(err).any()
    finally:
        bufs.close()


# ---------------------------------------------------------------- 3. a duplicated candidate
@pytest.mark.parametrize("W,H", SHAPES)
def test_a_duplicated_candidate_changes_nothing(gpu_ctx, W, H):
    rng, halves, rects, counts_a, counts_b, _, _, F, G, counts_f, _ = _inputs(W, H)
    bufs = _Select(gpu_ctx, halves, F, G)
    try:
        for r, f, k, alpha in CASES:
            c = _cands(k, alpha)
            for sw, lw in WINDOWS:
                kw = dict(radius=r, patch_radius=f, sure_window=sw, select_window=lw)
                once = bufs.run(rects, counts_a, counts_b, counts_f, c[:2], **kw)
                bufs.fill(rng)
                twice = bufs.run(rects, counts_a, counts_b, counts_f, [c[0], c[1], c[0], c[1]], **kw)
                for name in ("out", "err", "sure", "win"):
                    assert once[name].tobytes() == twice[name].tobytes(), (name, kw)
                alone = bufs.run(rects, counts_a, counts_b, counts_f, [c[1]], **kw)
                same = bufs.run(rects, counts_a, counts_b, counts_f, [c[1], c[1]], **kw)
                for name in ("out", "err", "sure", "win"):
                    assert alone[name].tobytes() == same[name].tobytes(), (name, kw)
                assert np.all(same["win"][~np.isnan(same["err"])] == 0)
    finally:
        bufs.close()


# ---------------------------------------------------------------- 4. window 0
@pytest.mark.parametrize("W,H", SHAPES)
def test_window_zero_hands_out_one_candidates_own_pixels(gpu_ctx, W, H):
    _, halves, rects, counts_a, counts_b, _, _, F, G, counts_f, _ = _inputs(W, H)
    bufs = _Select(gpu_ctx, halves, F, G)
    try:
        for r, f, k, alpha in CASES:
            cands = _cands(k, alpha)
            got = bufs.run(rects, counts_a, counts_b, counts_f, cands, radius=r, patch_radius=f, sure_window=0, select_window=0)
            own = [bufs.run(rects, counts_a, counts_b, counts_f, [c], radius=r, patch_radius=f, sure_window=0, select_window=0) for c in cands]
            dual = ~np.isnan(got["err"])
            assert np.all(got["win"][dual] < 4)
            for i in range(4):
                at = dual & (got["win"] == i)
                for name in ("out", "err", "sure"):
                    assert got[name][at].tobytes() == own[i][name][at].tobytes(), (name, i, r, f)
                if at.any():  # at window 0 the winner is the smallest per-pixel SURE itself
                    assert np.all(got["sure"][at] <= np.min([o["sure"][at] for o in own], axis=0))
            assert got["out"][~dual].tobytes() == own[0]["out"][~dual].tobytes()
    finally:
        bufs.close()


# ---------------------------------------------------------------- 5. radius 0
def test_radius_zero_is_the_closed_form_bit_for_bit(gpu_ctx):
    """r = 0: the only neighbour is the pixel itself, g = w / w = 1 and f = u, so t_c = ((0 * 0) - v_c) + ((2 * v_c) * 1) = v_c exactly: sure_X is the
    mean of v_X over the channels, and every candidate ties — candidate 0 wins."""
    W, H = 45, 29
    rng = np.random.default_rng(3)
    halves, rects, counts_a, counts_b, n_a, n_b = _two_halves(rng, W, H, 16, 8)
    F, G, counts_f, _ = _features(rng, W, H, rects)
    na, nb = n_a.astype(np.float64), n_b.astype(np.float64)
    u_a, v_a, ok_a = denoise_ref.mean_and_variance(halves[0], halves[1], n_a)
    u_b, v_b, ok_b = denoise_ref.mean_and_variance(halves[2], halves[3], n_b)
    dual = ok_a & ok_b
    with np.errstate(all="ignore"):
        out_x = np.where(dual[..., None], (na[..., None] * u_a + nb[..., None] * u_b) / (na + nb)[..., None], (halves[0] + halves[2]) / (na + nb)[..., None])
        h = (u_a - u_b) / 2.0
        err_x = np.where(dual, (h[..., 0] * h[..., 0] + h[..., 1] * h[..., 1] + h[..., 2] * h[..., 2]) / 3.0, np.nan)
        s_a, s_b = (((v[..., 0] + v[..., 1]) + v[..., 2]) / 3.0 for v in (v_a, v_b))
        sure_x = np.where(dual, (na * s_a + nb * s_b) / (na + nb), np.nan)
    bufs = _Select(gpu_ctx, halves, F, G)
    try:
        for f in (0, 1, 4):
            for sw, lw in ((0, 0), (2, 1)):
                got = bufs.run(rects, counts_a, counts_b, counts_f, _cands(0.45, 1.0), radius=0, patch_radius=f, sure_window=sw, select_window=lw)
                assert got["out"].tobytes() == out_x.tobytes() and got["err"].tobytes() == err_x.tobytes() and got["sure"].tobytes() == sure_x.tobytes()
                assert np.all(got["win"][dual] == 0) and np.all(got["win"][~dual] == sref.NO_WINNER)
        assert dual.any() and (~dual).any()
    finally:
        bufs.close()


# ---------------------------------------------------------------- 6. NULL outputs
@pytest.mark.parametrize("W,H", [(37, 23), (64, 48)])
def test_null_outputs_leave_the_others_unchanged(gpu_ctx, W, H):
    rng, halves, rects, counts_a, counts_b, _, _, F, G, counts_f, _ = _inputs(W, H)
    bufs = _Select(gpu_ctx, halves, F, G)
    try:
        for r, f, k, alpha in (CASES[2], CASES[3]):
            kw = dict(radius=r, patch_radius=f, sure_window=1, select_window=2)
            bufs.fill(rng)
            full = bufs.run(rects, counts_a, counts_b, counts_f, _cands(k, alpha), **kw)
            for want in (("sure", "win"), ("err", "win"), ("err", "sure"), ()):
                init = bufs.fill(rng)
                got = bufs.run(rects, counts_a, counts_b, counts_f, _cands(k, alpha), want=want, **kw)
                assert got["out"].tobytes() == full["out"].tobytes()
                for name in ("err", "sure", "win"):  # written as in the full call when wanted, untouched when NULL
                    assert got[name].tobytes() == (full if name in want else init)[name].tobytes(), (name, want)
    finally:
        bufs.close()


# ---------------------------------------------------------------- 7. the host paths
@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_render_tiled_with_dual_select_equals_the_direct_call(gpu_ctx, which, tmp_path):
    sc = _scene(which)
    tiles = generate_tiles(HW, HH, (32, 32))
    st = _settings(denoise_dual_select=True)
    handle = render.render_tiled(sc, st, devices=(0,))
    assert handle.scene is sc
    on_messages = [_message_key(m) for m in handle._messages]  # (await_() below consumes them)
    plain_st = Settings(scenes.camera(HW, HH), sample_count=HSPP, bounce_limit=HBOUNCES, seed=scenes.SEED)
    ds = render.DeviceScene(gpu_ctx, sc)
    try:
        halves = _direct_halves(gpu_ctx, ds, plain_st, tiles, HSPP // HSPI)
        F, G = _direct_features(gpu_ctx, ds, plain_st, tiles, [HSPP] * len(tiles))
    finally:
        ds.close()
    got_halves, rects, counts_a, counts_b = _assemble_dual(_finished_tiles(handle), HW, HH)
    assert rects == tiles and all(g.tobytes() == h.tobytes() for g, h in zip(got_halves, halves))
    cands = [dict(k=0.45, alpha=1.0), dict(k=1.0, alpha=1.0, guided=True, k_f=0.8, tau=2e-3)]  # _settings' denoise_feature_k and _tau
    assert st.select_candidates() == cands
    direct = render.denoise_dual_select_arrays(gpu_ctx, *halves, tiles, counts_a, counts_b, cands, features=F, features_sq=G, counts_f=[HSPP] * len(tiles),
                                               radius=5, patch_radius=2, sure_window=2, select_window=2)
    got = handle.await_()
    assert got.tobytes() == direct["out"].tobytes()
    wins = direct["win"].reshape(-1)
    assert 0 < (wins == 1).sum() < wins.size  # both candidates win somewhere: the frame is neither candidate's own
    # the setting off: the messages and the frame are those of denoise_dual alone
    off = render.render_tiled(sc, _settings(), devices=(0,))
    assert off.scene is None and [_message_key(m) for m in off._messages] == on_messages
    off.async_await()
    unguided, _ = render.denoise_dual_arrays(gpu_ctx, *halves, tiles, counts_a, counts_b, radius=5, patch_radius=2, k=0.45, alpha=1.0)
    assert off.await_().tobytes() == unguided.tobytes() and got.tobytes() != unguided.tobytes()
    # the C++ mirror
    cli = _cli()
    ppm, raw = tmp_path / "o.ppm", tmp_path / "o.f64"
    r = subprocess.run([cli, "render", "spheres" if which == "spheres" else "dragon:24", str(HW), str(HH), str(HSPP), str(HBOUNCES), str(ppm), "--raw", str(raw),
                        "--spi", str(HSPI), "--denoise", "1", "--denoise-dual", "1", "--denoise-dual-select", "1", "--denoise-radius", "5", "--denoise-patch", "2",
                        "--denoise-feature-k", "0.8", "--denoise-feature-tau", "0.002"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert np.fromfile(raw).reshape(HH, HW, 3).tobytes() == got.tobytes()
    assert os.path.samefile(cli, CLI)


# ---------------------------------------------------------------- 8, 9. quality and calibration on rendered frames
QW, QH, QSPP, QPASS, QBOUNCES, QREF = 256, 144, 32, 8, 5, 2048
_quality_cache = {}


def _quality(ctx, which):
    """256 x 144, 5 bounces, 32 spp in passes of 8 that alternate between the halves (A: samples 0-7 and 16-23, B: the others), the features of the
    same 32 samples, the shipped parameters and the default candidates, both windows 2; the reference is 2,048 spp of seed + 1.  Computed once per
    scene -> dict name -> (rmse, sqrt(mean sure) / rmse, sqrt(mean err) / rmse) for "select", "cand0", "cand1" """
    if which in _quality_cache:
        return _quality_cache[which]
    sc = _scene(which)
    tiles, whole = generate_tiles(QW, QH, (32, 32)), [(0, 0, QW, QH)]
    st = Settings(scenes.camera(QW, QH), sample_count=QSPP, bounce_limit=QBOUNCES, seed=scenes.SEED, samples_per_iteration=QPASS, denoise=True, denoise_dual=True,
                  denoise_dual_select=True)
    ref_st = Settings(scenes.camera(QW, QH), sample_count=QREF, bounce_limit=QBOUNCES, seed=scenes.SEED + 1)
    opened = [render.DeviceScene(ctx, sc)]
    res = {}
    try:
        ds = opened[0]
        fbs = [render.Framebuffer(ctx, QW, QH) for _ in range(5)]
        feat = [render.FeatureBuffer(ctx, QW, QH) for _ in range(2)]
        imgs = [render.ErrorImage(ctx, QW, QH) for _ in range(2)]
        opened += fbs + feat + imgs
        render.render_tiles(ctx, ds, ref_st.camera_settings, ref_st, tiles, fbs[4])
        ref = fbs[4].download() / float(QREF)
        for j in range(QSPP // QPASS):
            render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fbs[2 * (j & 1)], j * QPASS, QPASS, framebuffer_sq=fbs[2 * (j & 1) + 1])
        render.render_features(ctx, ds, st.camera_settings, st, tiles, feat[0], 0, QSPP, features_sq=feat[1])
        cands = st.select_candidates()
        assert cands == [dict(k=0.45, alpha=1.0), dict(k=1.0, alpha=1.0, guided=True, k_f=1.0, tau=1e-2)]
        for name, cs in (("select", cands), ("cand0", cands[:1]), ("cand1", cands[1:])):
            render.denoise_dual_select(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), whole, [QSPP // 2], [QSPP // 2], cs, fbs[4], imgs[0], imgs[1], None,
                                       radius=st.denoise_radius, patch_radius=st.denoise_patch, sure_window=2, select_window=2, features=feat[0],
                                       features_sq=feat[1], counts_f=[QSPP])
            rmse = float(np.sqrt(np.mean((fbs[4].download() - ref) ** 2)))
            err, sure = imgs[0].download(), imgs[1].download()
            assert np.isfinite(err).all() and np.isfinite(sure).all()
            res[name] = (rmse, float(np.sqrt(sure.mean())) / rmse, float(np.sqrt(err.mean())) / rmse)
    finally:
        for o in reversed(opened):
            o.close()
    _quality_cache[which] = res
    return res


@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_the_selected_frame_is_no_worse_than_its_candidates(gpu_ctx, which):
    """ReflectiveSpheres: RMSE(select) <= 1.0 x the SMALLER candidate's (a CPU prototype measured x0.86).  The mesh scene has no prototype: the hard
    bar there is 1.0 x the LARGER candidate's, which only a broken selection fails; the ratio against the smaller is printed."""
    q = _quality(gpu_ctx, which)
    sel, c0, c1 = q["select"][0], q["cand0"][0], q["cand1"][0]
    print("select quality: %s 256x144 32 spp: RMSE select %.5g unguided k 0.45 %.5g guided k 1.0 %.5g; select / smaller %.4f, / larger %.4f" %
          (which, sel, c0, c1, sel / min(c0, c1), sel / max(c0, c1)))
    assert sel <= (min(c0, c1) if which == "spheres" else max(c0, c1))


@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_sure_is_calibrated_where_err_reads_low(gpu_ctx, which):
    """Each candidate alone: sqrt(mean sure) / the true RMSE within [1 / 1.3, 1.3] (a CPU prototype measured 0.91 - 1.12; the margin covers the
    reference's own noise of about 0.009 in the RMSE), and closer to 1 than sqrt(mean err) / the true RMSE."""
    q = _quality(gpu_ctx, which)
    for name in ("cand0", "cand1"):
        rmse, s, e = q[name]
        print("select calibration: %s %s: true RMSE %.5g, sqrt(mean sure) / RMSE %.4f, sqrt(mean err) / RMSE %.4f" % (which, name, rmse, s, e))
    for name in ("cand0", "cand1"):
        rmse, s, e = q[name]
        assert 1.0 / 1.3 <= s <= 1.3, (name, s)
        assert abs(s - 1.0) < abs(e - 1.0), (name, s, e)
