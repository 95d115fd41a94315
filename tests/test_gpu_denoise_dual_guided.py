"""rmd_denoise_dual_guided and rmd_denoise_dual_guided_region on the device: the kernels against the numpy restatement
(tests/denoise_dual_guided_ref.py), the definition's exact identities (null and all-zero features, radius 0, equal halves against the device's
rmd_denoise_guided), the step edge below the noise, the region form with no tolerance, and the host paths (Python render_tiled / await_, the
C++ mirror through raymond_cli).

The frames, counts, poison and tolerance are test_gpu_denoise.py's and test_gpu_denoise_dual.py's own (imported from them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_dual_guided_ref as dgref
import denoise_guided_ref as gref
import denoise_ref
from raymond_amd import render, scenes
from raymond_amd.scene import Settings, generate_tiles, tile_array
from test_gpu_denoise import CASES, _agree, _finished_tiles, _moments, _poison, _tiles_with_counts
from test_gpu_denoise_dual import CLI, _assemble_dual, _cli, _two_halves
from test_gpu_denoise_dual_region import _bits, _expect, _mask, _message_key, _key, _random_bytes, _region_sets

pytestmark = pytest.mark.gpu


def _features(rng, W, H, rects, counts_f=None):
    """Random feature sums and sums of squares with their own per-rect counts — unless given: unrelated to the halves', a 0 and a 1 among them —
    and NaN / inf planted in F and in G.  -> F, G, counts_f, n_f"""
    if counts_f is None:
        counts_f = [int(c) for c in rng.integers(2, 100, len(rects))]
        if len(rects) >= 8:
            counts_f[6], counts_f[7] = 0, 1
    n_f = denoise_ref.count_image(W, H, rects, counts_f)
    y, x = np.mgrid[0:H, 0:W]
    f = rng.uniform(-1.0, 1.0, (H, W, 7))
    f[..., 3:6] = np.stack([np.where(x < W // 2, 0.8, 0.2), 0.2 + 0.0 * x, np.where(y < H // 2, 0.2, 0.8)], axis=-1)  # steps, as albedos have
    f[..., 6] = 3.0 + 0.01 * x + np.where(x % 13 < 6, 0.0, 0.5)
    f[(x + 2 * y) % 17 == 0] = 0.0  # misses
    n = np.maximum(n_f, 0).astype(np.float64)[..., None]
    sigma = rng.uniform(0.0, 0.05, (H, W, 1)) * (x % 5 == 0)[..., None]
    mean = f + rng.normal(0.0, 1.0, (H, W, 7)) * sigma
    F = mean * n
    G = F * mean + rng.uniform(0.0, 1.0, (H, W, 7)) * sigma * sigma * np.maximum(n - 1.0, 0.0)
    if W * H > 1:
        for value, arr in ((np.nan, F), (np.inf, F), (np.inf, G), (np.nan, G)):
            for _ in range(max(1, H * W // 300)):
                arr[rng.integers(0, H), rng.integers(0, W), rng.integers(0, 7)] = value
    return F, G, counts_f, n_f


class _Buffers:
    """The two halves and the features uploaded once; out and err re-filled before each call."""

    def __init__(self, ctx, halves, F=None, G=None):
        self.ctx = ctx
        H, W = halves[0].shape[:2]
        self.fbs = [render.Framebuffer(ctx, W, H) for _ in range(5)]
        self.err = render.ErrorImage(ctx, W, H)
        self.feat = [None, None]
        for fb, arr in zip(self.fbs, halves):
            fb.upload(arr)
        if F is not None:
            self.feat = [render.FeatureBuffer(ctx, W, H), render.FeatureBuffer(ctx, W, H)]
            self.feat[0].upload(F), self.feat[1].upload(G)

    def run(self, rects, counts_a, counts_b, counts_f, region=None, out_init=None, err_init=None, with_err=True, guided=True, **params):
        if out_init is not None:
            self.fbs[4].upload(out_init), self.err.upload(err_init)
        kw = dict(features=self.feat[0], features_sq=self.feat[1], counts_f=counts_f) if guided else {}
        render.denoise_dual(self.ctx, (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3]), rects, counts_a, counts_b, self.fbs[4],
                            self.err if with_err else None, region=region, **kw, **params)
        return self.fbs[4].download(), self.err.download()

    def run_null(self, rects, counts_a, counts_b, region, out_init, err_init, **params):
        """The guided entry points themselves with feat_dev = feat_sq_dev = NULL, and a NULL rect_counts_f, a NaN k_f and a negative tau, which are
        then not read (render.denoise_dual makes the unguided calls when it has no features)."""
        self.fbs[4].upload(out_init), self.err.upload(err_init)
        ca, cb = (np.ascontiguousarray(c, dtype=np.uint32) for c in (counts_a, counts_b))
        L, u32 = self.ctx.L, C.POINTER(C.c_uint32)
        head = (self.ctx.handle, *(fb.ptr for fb in self.fbs[:4]), None, None, self.fbs[0].width, self.fbs[0].height, tile_array(rects), ca.ctypes.data_as(u32),
                cb.ctypes.data_as(u32), None, len(rects))
        tail = (params["radius"], params["patch_radius"], params["k"], params["alpha"], float("nan"), -1.0, self.fbs[4].ptr, self.err.ptr)
        if region is None:
            self.ctx.check(L.rmd_denoise_dual_guided(*head, *tail))
        else:
            self.ctx.check(L.rmd_denoise_dual_guided_region(*head, tile_array(region), len(region), *tail))
        return self.fbs[4].download(), self.err.download()

    def close(self):
        for b in self.fbs + [self.err] + [f for f in self.feat if f is not None]:
            b.close()


def _inputs(W, H):
    rng = np.random.default_rng(W * 1000 + H + 19)
    halves, rects, counts_a, counts_b, n_a, n_b = _two_halves(rng, W, H)  # poisoned sums, unequal counts with 0 and 1, one tile uncovered
    F, G, counts_f, n_f = _features(rng, W, H, rects)
    return rng, halves, rects, counts_a, counts_b, n_a, n_b, F, G, counts_f, n_f


# ---------------------------------------------------------------- the kernel against the restatement
@pytest.mark.parametrize("W,H", [(1, 1), (5, 200), (37, 23), (64, 48)])
def test_guided_dual_kernel_matches_the_restatement(gpu_ctx, W, H):
    _, halves, rects, counts_a, counts_b, n_a, n_b, F, G, counts_f, n_f = _inputs(W, H)
    bufs = _Buffers(gpu_ctx, halves, F, G)
    try:
        for r, f, k, alpha in CASES:
            for k_f, tau in ((1.0, 1e-2), (0.6, 1e-3)):
                params = dict(radius=r, patch_radius=f, k=k, alpha=alpha, k_f=k_f, tau=tau)
                out, err = bufs.run(rects, counts_a, counts_b, counts_f, **params)
                out_ref, err_ref = dgref.denoise_dual_guided(*halves, n_a, n_b, F, G, n_f, **params)
                _agree(out, out_ref)  # (NaN exactly where the restatement has NaN)
                _agree(err, err_ref)
                if r == 3 and W * H > 100:  # the features mattered
                    plain, _ = dgref.denoise_dual_guided(*halves, n_a, n_b, radius=r, patch_radius=f, k=k, alpha=alpha)
                    assert not np.array_equal(out_ref, plain, equal_nan=True)
    finally:
        bufs.close()


@pytest.mark.parametrize("W,H", [(37, 23), (70, 41)])
def test_null_and_all_zero_features_are_rmd_denoise_dual_bit_for_bit(gpu_ctx, W, H):
    rng, halves, rects, counts_a, counts_b, *_ = _inputs(W, H)
    Z = np.zeros((H, W, 7))
    twos = [2 + i % 5 for i in range(len(rects))]  # counts >= 2: every dual-valid pixel is feature-valid, and w_f = exp(-0) = 1 never cuts a weight
    out_init, err_init = _random_bytes(rng, (H, W, 3)), _random_bytes(rng, (H, W))
    region = _region_sets(W, H)["unaligned"]
    zero, null = _Buffers(gpu_ctx, halves, Z, Z), _Buffers(gpu_ctx, halves)
    try:
        for r, f, k, alpha in CASES:
            params = dict(radius=r, patch_radius=f, k=k, alpha=alpha)
            for reg in (None, region):
                want = null.run(rects, counts_a, counts_b, None, reg, out_init, err_init, guided=False, **params)  # rmd_denoise_dual[_region]
                got_null = null.run_null(rects, counts_a, counts_b, reg, out_init, err_init, **params)
                got_zero = zero.run(rects, counts_a, counts_b, twos, reg, out_init, err_init, **params)
                for got in (got_null, got_zero):
                    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (params, reg is None)
        assert np.isnan(want[1]).any() and np.isfinite(want[1]).any()
    finally:
        zero.close(), null.close()


def test_radius_zero_is_the_closed_form_bit_for_bit(gpu_ctx):
    W, H = 45, 29
    rng = np.random.default_rng(3)
    halves, rects, counts_a, counts_b, n_a, n_b = _two_halves(rng, W, H, 16, 8)
    F, G, counts_f, _ = _features(rng, W, H, rects)
    na, nb = n_a.astype(np.float64)[..., None], n_b.astype(np.float64)[..., None]
    _, _, ok_a = denoise_ref.mean_and_variance(halves[0], halves[1], n_a)
    _, _, ok_b = denoise_ref.mean_and_variance(halves[2], halves[3], n_b)
    dual = ok_a & ok_b
    with np.errstate(all="ignore"):
        u_a, u_b = halves[0] / na, halves[2] / nb
        out_x = np.where(dual[..., None], (na * u_a + nb * u_b) / (na + nb), (halves[0] + halves[2]) / (na + nb))
        h = (u_a - u_b) / 2.0
        err_x = np.where(dual, (h[..., 0] * h[..., 0] + h[..., 1] * h[..., 1] + h[..., 2] * h[..., 2]) / 3.0, np.nan)
    bufs = _Buffers(gpu_ctx, halves, F, G)
    try:
        for f in (0, 1, 4):
            out, err = bufs.run(rects, counts_a, counts_b, counts_f, radius=0, patch_radius=f)
            assert out.tobytes() == out_x.tobytes() and err.tobytes() == err_x.tobytes()
    finally:
        bufs.close()


@pytest.mark.parametrize("n", [8, 12])
def test_equal_halves_give_the_device_rmd_denoise_guided_and_no_error(gpu_ctx, n):
    """A == B and counts_f == counts: err == 0 exactly; out is rmd_denoise_guided of that half on the device bit for bit at a power-of-two count,
    and within the one rounding of n * f that the stated operation order leaves at any other (raymond_hip.h)."""
    rng = np.random.default_rng(4)
    W, H = 70, 41
    rects = generate_tiles(W, H, (32, 16))
    counts = [n] * len(rects)
    counts[2] = 1  # a tile that is not valid
    n_img = denoise_ref.count_image(W, H, rects, counts)
    S, Q = _moments(rng, n_img)
    _poison(S, Q, rng)
    F, G, _, _ = _features(rng, W, H, rects, counts)  # at the halves' own counts
    _, _, valid = denoise_ref.mean_and_variance(S, Q, n_img)
    bufs = _Buffers(gpu_ctx, (S, Q, S, Q), F, G)
    try:
        for r, f in ((1, 0), (4, 2), (10, 3), (12, 4)):  # both tile widths
            out, err = bufs.run(rects, counts, counts, counts, radius=r, patch_radius=f)
            single = render.denoise_guided_arrays(gpu_ctx, S, Q, F, G, rects, counts, radius=r, patch_radius=f)
            assert np.all(err[valid] == 0.0) and np.isnan(err[~valid]).all()
            if n == 8:
                assert out[valid].tobytes() == single[valid].tobytes()
            else:
                assert np.all(np.abs(out[valid] - single[valid]) <= np.spacing(np.abs(single[valid])))
            if r >= 4:  # the features mattered
                assert single.tobytes() != render.denoise_arrays(gpu_ctx, S, Q, rects, counts, radius=r, patch_radius=f).tobytes()
    finally:
        bufs.close()


def test_hit_miss_frame_as_both_halves_is_exact(gpu_ctx):
    S, Q, F, G, n, u = gref.hit_miss_frame()
    H, W = n.shape
    rect, c = [(0, 0, W, H)], [int(n[0, 0])]
    out, err = render.denoise_dual_arrays(gpu_ctx, S, Q, S, Q, rect, c, c, features=F + F, features_sq=G + G, counts_f=[2 * c[0]])
    assert out.tobytes() == u.tobytes() and np.all(err == 0.0)
    un, _ = render.denoise_dual_arrays(gpu_ctx, S, Q, S, Q, rect, c, c)
    assert np.abs(un - u).max() > 0.2  # the colour weights alone mix across the step


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_step_edge_on_the_device(gpu_ctx, seed):
    """Halves step_edge_frame(seed) and (seed + 1000), the features of A added to themselves at a count of 32, r = 10, f = 3, k = 0.45, alpha = 1,
    k_f = 1.0, tau = 1e-2.  The restatement gives 0.21 - 0.31 of rmd_denoise_dual's band RMSE; the bar is 0.5."""
    S_a, Q_a, F, G, n, truth = gref.step_edge_frame(seed)
    S_b, Q_b = gref.step_edge_frame(seed + 1000)[:2]
    H, W = n.shape
    rect, c = [(0, 0, W, H)], [int(n[0, 0])]
    params = dict(radius=10, patch_radius=3, k=0.45, alpha=1.0)
    gd, _ = render.denoise_dual_arrays(gpu_ctx, S_a, Q_a, S_b, Q_b, rect, c, c, features=F + F, features_sq=G + G, counts_f=[2 * c[0]], k_f=1.0, tau=1e-2,
                                       **params)
    un, _ = render.denoise_dual_arrays(gpu_ctx, S_a, Q_a, S_b, Q_b, rect, c, c, **params)
    rg, ru = gref.band_rmse(gd, truth), gref.band_rmse(un, truth)
    print("step edge on the device, seed %d: band RMSE guided dual %.5f rmd_denoise_dual %.5f ratio %.3f" % (seed, rg, ru, rg / ru))
    assert rg <= 0.5 * ru


# ---------------------------------------------------------------- the region form: no tolerance
@pytest.mark.parametrize("W,H", [(37, 23), (200, 120)])
def test_region_equals_the_full_frame_and_nothing_else_is_written(gpu_ctx, W, H):
    rng, halves, rects, counts_a, counts_b, _, _, F, G, counts_f, _ = _inputs(W, H)
    out_init, err_init = _random_bytes(rng, (H, W, 3)), _random_bytes(rng, (H, W))
    bufs = _Buffers(gpu_ctx, halves, F, G)
    try:
        for r, f, k, alpha in (CASES[1], CASES[3], CASES[4]):  # r = 1; the 32-wide tile at r = 10, f = 3; the 24-wide one at r = 12, f = 4
            params = dict(radius=r, patch_radius=f, k=k, alpha=alpha, k_f=0.6, tau=1e-3)
            full_out, full_err = bufs.run(rects, counts_a, counts_b, counts_f, None, out_init, err_init, **params)
            for name, region in _region_sets(W, H).items():
                mask = _mask(W, H, region)
                out, err = bufs.run(rects, counts_a, counts_b, counts_f, region, out_init, err_init, **params)
                assert _bits(out).tobytes() == _expect(mask, full_out, out_init).tobytes(), (name, params)
                assert _bits(err).tobytes() == _expect(mask, full_err, err_init).tobytes(), (name, params)
                out, err = bufs.run(rects, counts_a, counts_b, counts_f, region, out_init, err_init, with_err=False, **params)  # err_dev = NULL
                assert _bits(out).tobytes() == _expect(mask, full_out, out_init).tobytes(), (name, params)
                assert err.tobytes() == err_init.tobytes(), (name, params)
        assert np.isnan(full_err).any() and np.isfinite(full_err).any()
        plain, _ = bufs.run(rects, counts_a, counts_b, None, None, out_init, err_init, guided=False, radius=r, patch_radius=f, k=k, alpha=alpha)
        assert plain.tobytes() != full_out.tobytes()  # the features mattered
    finally:
        bufs.close()


@pytest.mark.parametrize("W,H", [(37, 23), (200, 120)])
def test_two_disjoint_calls_compose_to_the_full_frame_in_both_orders(gpu_ctx, W, H):
    rng, halves, rects, counts_a, counts_b, _, _, F, G, counts_f, _ = _inputs(W, H)
    out_init, err_init = _random_bytes(rng, (H, W, 3)), _random_bytes(rng, (H, W))
    tiles = generate_tiles(W, H, (8, 16))
    bufs = _Buffers(gpu_ctx, halves, F, G)
    try:
        for r, f, k, alpha in (CASES[3], CASES[4]):
            params = dict(radius=r, patch_radius=f, k=k, alpha=alpha)
            full_out, full_err = bufs.run(rects, counts_a, counts_b, counts_f, None, out_init, err_init, **params)
            for first, second in ((tiles[::2], tiles[1::2]), (tiles[1::2], tiles[::2])):
                bufs.run(rects, counts_a, counts_b, counts_f, first, out_init, err_init, **params)
                out, err = bufs.run(rects, counts_a, counts_b, counts_f, second, **params)  # into the buffers as the first call left them
                assert out.tobytes() == full_out.tobytes() and err.tobytes() == full_err.tobytes(), (params, len(first))
    finally:
        bufs.close()


# ---------------------------------------------------------------- the host paths
HW, HH, HSPP, HSPI, HBOUNCES = 96, 64, 32, 8, 4
HPARAMS = dict(radius=5, patch_radius=2, k=0.45, alpha=1.0)
HGUIDE = dict(k_f=0.8, tau=2e-3)


def _scene(which):
    return scenes.reflective_spheres() if which == "spheres" else scenes.gold_dragon_standin(n=24)


def _settings(**kw):
    return Settings(scenes.camera(HW, HH), sample_count=HSPP, tile_size=(32, 32), bounce_limit=HBOUNCES, seed=scenes.SEED, samples_per_iteration=HSPI,
                    denoise=True, denoise_dual=True, denoise_radius=5, denoise_patch=2, denoise_feature_k=0.8, denoise_feature_tau=2e-3, **kw)


def _direct_halves(ctx, ds, st, tiles, n_passes):
    """rmd_render_tiles_moments into two halves by pass parity: pass j covers samples [j * spi, (j + 1) * spi) and goes to A when j is even."""
    fbs = [render.Framebuffer(ctx, HW, HH) for _ in range(4)]
    try:
        for j in range(n_passes):
            render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fbs[2 * (j & 1)], j * HSPI, HSPI, framebuffer_sq=fbs[2 * (j & 1) + 1])
        return [fb.download() for fb in fbs]
    finally:
        for fb in fbs:
            fb.close()


def _direct_features(ctx, ds, st, rects, counts):
    """rmd_render_features over [0, n) per rect, into fresh buffers."""
    fb, fb_sq = render.FeatureBuffer(ctx, HW, HH), render.FeatureBuffer(ctx, HW, HH)
    try:
        for r, c in zip(rects, counts):
            render.render_features(ctx, ds, st.camera_settings, st, [r], fb, 0, c, features_sq=fb_sq)
        return fb.download(), fb_sq.download()
    finally:
        fb.close(), fb_sq.close()


@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_render_tiled_with_dual_features_equals_the_direct_calls(gpu_ctx, which, tmp_path):
    sc = _scene(which)
    tiles = generate_tiles(HW, HH, (32, 32))
    st = _settings(denoise_dual_features=True)
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
    assert rects == tiles and set(counts_a) == set(counts_b) == {HSPP // 2}
    assert all(g.tobytes() == h.tobytes() for g, h in zip(got_halves, halves))
    assert F.any()
    expected, _ = render.denoise_dual_arrays(gpu_ctx, *halves, tiles, counts_a, counts_b, features=F, features_sq=G, counts_f=[HSPP] * len(tiles), **HPARAMS,
                                             **HGUIDE)
    got = handle.await_()
    assert got.tobytes() == expected.tobytes()
    unguided, _ = render.denoise_dual_arrays(gpu_ctx, *halves, tiles, counts_a, counts_b, **HPARAMS)
    assert got.tobytes() != unguided.tobytes()
    # the setting off: the dual render's messages and frame are those of denoise_dual alone — what the same call gave before the setting existed
    off = render.render_tiled(sc, _settings(), devices=(0,))
    assert off.scene is None
    assert len(on_messages) == 4 * len(tiles) and [_message_key(m) for m in off._messages] == on_messages  # (the features change no message)
    off.async_await()
    assert off.await_().tobytes() == unguided.tobytes()
    # the C++ mirror
    cli = _cli()
    ppm, raw = tmp_path / "o.ppm", tmp_path / "o.f64"
    r = subprocess.run([cli, "render", "spheres" if which == "spheres" else "dragon:24", str(HW), str(HH), str(HSPP), str(HBOUNCES), str(ppm), "--raw", str(raw),
                        "--spi", str(HSPI), "--denoise", "1", "--denoise-dual", "1", "--denoise-dual-features", "1", "--denoise-radius", "5", "--denoise-patch", "2",
                        "--denoise-feature-k", "0.8", "--denoise-feature-tau", "0.002"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert np.fromfile(raw).reshape(HH, HW, 3).tobytes() == got.tobytes()
    assert os.path.samefile(cli, CLI)


def _reenact(ctx, sc, st, guided):
    """The adaptive dual-buffer loop restated with the WHOLE-FRAME call: after every even number of passes that leaves live tiles below sample_count
    with at least adaptive_min_samples, render.denoise_dual over the whole frame (guided: with the features of the same samples at count_a +
    count_b) and render.tile_error_dual over the live tiles.  -> the messages as _key tuples, the number of checks"""
    cam = st.camera_settings
    ds = render.DeviceScene(ctx, sc)
    fbs = [render.Framebuffer(ctx, HW, HH) for _ in range(5)]
    feat = [render.FeatureBuffer(ctx, HW, HH) for _ in range(2)]
    err_img = render.ErrorImage(ctx, HW, HH)
    progressed, finished, checks = [], [], 0
    try:
        live = generate_tiles(HW, HH, st.tile_size)
        done_rects, done_a, done_b = [], [], []
        n_half, done, j = [0, 0], 0, 0

        def finish(imgs, rect, error):
            l, t, w, h = rect
            a, a_sq, b, b_sq = (img[t : t + h, l : l + w] for img in imgs)
            finished.append(_key("TileFinished", rect, n_half[0] + n_half[1], error, a + b, a_sq + b_sq, a, a_sq, b, b_sq, n_half[0], n_half[1]))
            done_rects.append(rect), done_a.append(n_half[0]), done_b.append(n_half[1])

        while done < st.sample_count and live:
            n = min(st.samples_per_iteration, st.sample_count - done)
            half = j & 1
            render.render_tiles(ctx, ds, cam, st, live, fbs[2 * half], done, n, framebuffer_sq=fbs[2 * half + 1])
            if guided:
                render.render_features(ctx, ds, cam, st, live, feat[0], done, n, features_sq=feat[1])
            done, j = done + n, j + 1
            n_half[half] += n
            if done < st.sample_count:
                errors = [None] * len(live)
                if j % 2 == 0 and done >= st.adaptive_min_samples:
                    checks += 1
                    ca, cb = done_a + [n_half[0]] * len(live), done_b + [n_half[1]] * len(live)
                    kw = dict(features=feat[0], features_sq=feat[1], counts_f=[a + b for a, b in zip(ca, cb)], **HGUIDE) if guided else {}
                    render.denoise_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), done_rects + live, ca, cb, fbs[4], err_img, **HPARAMS, **kw)
                    errors = [float(e) for e in render.tile_error_dual(ctx, err_img, live)]
                imgs = [fb.download() for fb in fbs[:4]]
                still = []
                for rect, e in zip(live, errors):
                    if e is not None and e <= st.adaptive_denoised_threshold:
                        finish(imgs, rect, e)
                    else:
                        l, t, w, h = rect
                        progressed.append(_key("TileProgressed", rect, done, e, imgs[0][t : t + h, l : l + w] + imgs[2][t : t + h, l : l + w]))
                        still.append(rect)
                live = still
        imgs = [fb.download() for fb in fbs[:4]]
        for rect in live:
            finish(imgs, rect, None)
    finally:
        for o in fbs + feat + [err_img, ds]:
            o.close()
    return progressed + finished, checks


@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_the_adaptive_render_with_dual_features_sends_the_reenactments_messages(gpu_ctx, which, tmp_path):
    """Threshold: the median rmd_tile_error_dual of the guided whole-frame call at the first check (16 samples), so that some tiles finish there and
    others go on; checks at 16 samples (adaptive_min_samples 16)."""
    sc = _scene(which)
    tiles = generate_tiles(HW, HH, (32, 32))
    plain_st = Settings(scenes.camera(HW, HH), sample_count=HSPP, bounce_limit=HBOUNCES, seed=scenes.SEED)
    ds = render.DeviceScene(gpu_ctx, sc)
    try:
        halves = _direct_halves(gpu_ctx, ds, plain_st, tiles, 2)
        F, G = _direct_features(gpu_ctx, ds, plain_st, tiles, [2 * HSPI] * len(tiles))
    finally:
        ds.close()
    fbs = [render.Framebuffer(gpu_ctx, HW, HH) for _ in range(5)]
    err = render.ErrorImage(gpu_ctx, HW, HH)
    feat = [render.FeatureBuffer(gpu_ctx, HW, HH) for _ in range(2)]
    try:
        for fb, arr in zip(fbs[:4] + feat, halves + [F, G]):
            fb.upload(arr)
        c = [HSPI] * len(tiles)
        render.denoise_dual(gpu_ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), tiles, c, c, fbs[4], err, features=feat[0], features_sq=feat[1],
                            counts_f=[2 * HSPI] * len(tiles), **HPARAMS, **HGUIDE)
        threshold = float(np.median(render.tile_error_dual(gpu_ctx, err, tiles)))
    finally:
        for o in fbs + feat + [err]:
            o.close()
    st = _settings(denoise_dual_features=True, adaptive_denoised_threshold=threshold, adaptive_min_samples=16)
    expected, checks = _reenact(gpu_ctx, sc, st, guided=True)
    counts = [m[2] for m in expected if m[0] == "TileFinished"]
    print("guided adaptive render (%s): threshold %.6g, %d checks, finished at %s" % (which, threshold, checks, sorted(counts)))
    assert min(counts) < HSPP and max(counts) == HSPP, "the adaptive form was not exercised"
    handle = render.render_tiled(sc, st, devices=(0,))
    got = [_message_key(m) for m in handle._messages]
    assert len(got) == len(expected)
    for g, e in zip(got, expected):
        assert g == e, (g[:4], e[:4])
    # await_'s frame: the whole-frame guided call over the finished tiles, each tile's features at count_a + count_b
    fin = _finished_tiles(handle)
    fhalves, rects, counts_a, counts_b = _assemble_dual(fin, HW, HH)
    counts_f = [a + b for a, b in zip(counts_a, counts_b)]
    ds = render.DeviceScene(gpu_ctx, sc)
    try:
        F, G = _direct_features(gpu_ctx, ds, plain_st, rects, counts_f)
    finally:
        ds.close()
    frame, _ = render.denoise_dual_arrays(gpu_ctx, *fhalves, rects, counts_a, counts_b, features=F, features_sq=G, counts_f=counts_f, **HPARAMS, **HGUIDE)
    img = handle.await_()
    assert img.tobytes() == frame.tobytes()
    # the setting off under the same threshold: the unguided re-enactment's messages (the parent's code path)
    st_off = _settings(adaptive_denoised_threshold=threshold, adaptive_min_samples=16)
    expected_off, _ = _reenact(gpu_ctx, sc, st_off, guided=False)
    assert [_message_key(m) for m in render.render_tiled(sc, st_off, devices=(0,))._messages] == expected_off
    # the C++ mirror calls the guided region form and writes the same frame
    cli = _cli()
    undefined = subprocess.run(["nm", "-D", "--undefined-only", cli], check=True, capture_output=True, text=True).stdout
    assert "rmd_denoise_dual_guided_region" in undefined and "rmd_denoise_dual_guided\n" in undefined
    ppm, raw = tmp_path / "o.ppm", tmp_path / "o.f64"
    r = subprocess.run([cli, "render", "spheres" if which == "spheres" else "dragon:24", str(HW), str(HH), str(HSPP), str(HBOUNCES), str(ppm), "--raw", str(raw),
                        "--spi", str(HSPI), "--denoise", "1", "--denoise-dual", "1", "--denoise-dual-features", "1", "--denoise-radius", "5", "--denoise-patch", "2",
                        "--denoise-feature-k", "0.8", "--denoise-feature-tau", "0.002", "--adaptive-denoised", "%.17g" % threshold, "--adaptive-min", "16"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert np.fromfile(raw).reshape(HH, HW, 3).tobytes() == frame.tobytes()


# ---------------------------------------------------------------- quality on real renders
@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_guided_dual_at_its_defaults_is_no_worse_than_rmd_denoise_dual(gpu_ctx, which):
    """test_gpu_denoise_dual.py's size and counts — 256 x 144, 5 bounces, 32 + 32 samples (A: samples 0 .. 31, B: 32 .. 63), RMSE in linear radiance
    against the 2,048 spp frame of seed + 1 — with the features of the same 64 samples and the shipped parameters; the comparator is
    rmd_denoise_dual on the same halves, the bar 1.0.  (tools/dual_guided_quality.py measured 0.0149 against 0.0156 on ReflectiveSpheres and 0.0169
    against 0.0182 on the mesh scene: DESIGN.md section 15.)"""
    W, H, half, bounces = 256, 144, 32, 5
    sc = _scene(which)
    tiles, whole = generate_tiles(W, H, (32, 32)), [(0, 0, W, H)]
    st = Settings(scenes.camera(W, H), sample_count=2 * half, bounce_limit=bounces, seed=scenes.SEED)
    ref_st = Settings(scenes.camera(W, H), sample_count=2048, bounce_limit=bounces, seed=scenes.SEED + 1)
    opened = [render.DeviceScene(gpu_ctx, sc)]
    try:
        ds = opened[0]
        fbs = [render.Framebuffer(gpu_ctx, W, H) for _ in range(5)]
        feat = [render.FeatureBuffer(gpu_ctx, W, H) for _ in range(2)]
        opened += fbs + feat
        render.render_tiles(gpu_ctx, ds, ref_st.camera_settings, ref_st, tiles, fbs[4])
        ref = fbs[4].download() / 2048.0
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fbs[0], 0, half, framebuffer_sq=fbs[1])
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fbs[2], half, half, framebuffer_sq=fbs[3])
        render.render_features(gpu_ctx, ds, st.camera_settings, st, tiles, feat[0], 0, 2 * half, features_sq=feat[1])
        params = dict(radius=st.denoise_radius, patch_radius=st.denoise_patch, k=st.denoise_k, alpha=st.denoise_alpha)  # the shipped defaults
        render.denoise_dual(gpu_ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), whole, [half], [half], fbs[4], **params)
        un = float(np.sqrt(np.mean((fbs[4].download() - ref) ** 2)))
        render.denoise_dual(gpu_ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), whole, [half], [half], fbs[4], features=feat[0], features_sq=feat[1], counts_f=[2 * half],
                            k_f=st.denoise_feature_k, tau=st.denoise_feature_tau, **params)
        gd = float(np.sqrt(np.mean((fbs[4].download() - ref) ** 2)))
    finally:
        for o in reversed(opened):
            o.close()
    print("guided dual quality: %s 256x144 32 + 32 spp: RMSE rmd_denoise_dual %.5g guided %.5g ratio %.4f" % (which, un, gd, gd / un))
    assert gd <= un, (gd, un)
