"""rmd_denoise_atrous_dual_region on the device: inside the region the bytes of rmd_denoise_atrous_dual, outside it nothing written — also when the
scratch memory the context keeps is full of another frame's planes —; disjoint calls compose to the whole frame; the scratch grows with the frame; and
the adaptive dual-buffer render (Python and raymond_cli) with denoise_dual_atrous_region checks its live tiles through the region form and sends what
it sends without the setting.

No tolerance anywhere: every comparison is equality of bits between two device results."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_denoise as tgd
from raymond_amd import abi, render, scenes
from raymond_amd.scene import Settings, generate_tiles
from test_gpu_denoise_atrous_dual import CLI_ARGS, HBOUNCES, HGUIDE, HH, HSPI, HW, _scene
from test_gpu_denoise_dual import CLI, _cli, _two_halves
from test_gpu_denoise_dual_guided import _features
from test_gpu_denoise_dual_region import _bits, _clip, _expect, _mask, _message_key, _random_bytes

pytestmark = pytest.mark.gpu

# 1 x 1; narrower than a workgroup's 64 x 4 block; two blocks across and three down; wider than twice the 5-level reach of 62 pixels, so that a small
# region leaves blocks that no level computes
FRAMES = [(1, 1), (7, 5), (70, 9), (200, 120)]
LEVELS = (0, 1, 3, 5, abi.RMD_ATROUS_MAX_LEVELS)
GUIDE = dict(k_f=0.6, tau=1e-3)
FILTER = dict(k=3.0, alpha=1.0)


def _inputs(W, H, salt):
    """test_gpu_denoise_atrous_dual's recipe: poisoned sums, unequal counts with 0 and 1, one tile uncovered, features with NaN / inf at counts of their own."""
    rng = np.random.default_rng(W * 1000 + H + salt)
    halves, rects, counts_a, counts_b, _, _ = _two_halves(rng, W, H)
    F, G, counts_f, _ = _features(rng, W, H, rects)
    return rng, halves, rects, counts_a, counts_b, F, G, counts_f


class _Buffers:
    """The two halves and the features uploaded once; out and err filled before each call."""

    def __init__(self, ctx, W, H, salt):
        self.ctx, self.shape = ctx, (H, W)
        self.rng, halves, self.rects, self.counts_a, self.counts_b, F, G, self.counts_f = _inputs(W, H, salt)
        self.fbs = [render.Framebuffer(ctx, W, H) for _ in range(5)]
        self.err = render.ErrorImage(ctx, W, H)
        self.feat = [render.FeatureBuffer(ctx, W, H), render.FeatureBuffer(ctx, W, H)]
        for fb, arr in zip(self.fbs, halves):
            fb.upload(arr)
        self.feat[0].upload(F), self.feat[1].upload(G)

    def call(self, region, guided, with_err=True, **params):
        kw = dict(features=self.feat[0], features_sq=self.feat[1], counts_f=self.counts_f, **GUIDE) if guided else {}
        render.denoise_atrous_dual(self.ctx, (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3]), self.rects, self.counts_a, self.counts_b, self.fbs[4],
                                   self.err if with_err else None, region=region, **kw, **FILTER, **params)

    def run(self, region, guided, out_init, err_init, with_err=True, **params):
        self.fbs[4].upload(out_init), self.err.upload(err_init)
        self.call(region, guided, with_err, **params)
        return self.fbs[4].download(), self.err.download()

    def close(self):
        for b in self.fbs + [self.err] + self.feat:
            b.close()


def _region_sets(W, H, poison):
    corners = sorted({(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1)})
    sets = {"whole_frame": [(0, 0, W, H)],
            "every_other_8x16_tile": generate_tiles(W, H, (8, 16))[::2],
            "corners": corners,
            # aligned to neither the 64 x 4 block nor the rects, wider and higher than one block, pairwise disjoint
            "unaligned": _clip([(3, 5, 41, 19), (47, 1, 29, 37), (1, 27, 45, 17), (101, 33, 77, 55)], W, H),
            "empty": [],
            "centre": [(W // 2, H // 2, 1, 1)]}
    if poison is not None:  # a pixel that is not dual-valid: as the region, and one tap of level 0 away from it
        x, y = poison
        sets["poisoned_pixel"] = [(x, y, 1, 1)]
        sets["beside_a_poisoned_pixel"] = [(x + 1, y, 1, 1)] if x + 1 < W else [(x - 1, y, 1, 1)]
    return sets


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("W,H", FRAMES)
def test_region_equals_the_whole_frame_over_stale_scratch_and_nothing_else_is_written(gpu_ctx, W, H, guided):
    """Per case: (1) a region call over the whole frame on OTHER inputs of the same size, which leaves the context's scratch full of wrong planes — what
    a level computed on too small a set would read; (2) the region call under test into out / err filled with random bytes; (3) the whole-frame call;
    (4) the region call's bits are the whole-frame call's inside the region and the fill's outside."""
    bufs, other = _Buffers(gpu_ctx, W, H, 23), _Buffers(gpu_ctx, W, H, 77)
    rng = bufs.rng
    out_init, err_init = _random_bytes(rng, (H, W, 3)), _random_bytes(rng, (H, W))
    try:
        for levels in LEVELS:
            full_out, full_err = bufs.run(None, guided, out_init, err_init, levels=levels)
            bad = np.argwhere(np.isnan(full_err))
            poison = None if len(bad) == 0 or W * H == 1 else (int(bad[len(bad) // 2][1]), int(bad[len(bad) // 2][0]))
            for name, region in _region_sets(W, H, poison).items():
                other.call([(0, 0, W, H)], guided, levels=levels)
                out, err = bufs.run(region, guided, out_init, err_init, levels=levels)
                mask = _mask(W, H, region)
                assert _bits(out).tobytes() == _expect(mask, full_out, out_init).tobytes(), (name, levels)
                assert _bits(err).tobytes() == _expect(mask, full_err, err_init).tobytes(), (name, levels)
            if W * H > 600:  # the inputs make the comparison mean something
                assert poison is not None and np.isfinite(full_err).any()
                assert not np.array_equal(_bits(full_out), _bits(other.run(None, guided, out_init, err_init, levels=levels)[0]))
    finally:
        bufs.close(), other.close()


@pytest.mark.parametrize("W,H", [(70, 9), (200, 120)])
def test_two_disjoint_calls_compose_to_the_whole_frame_in_both_orders(gpu_ctx, W, H):
    bufs = _Buffers(gpu_ctx, W, H, 23)
    out_init, err_init = _random_bytes(bufs.rng, (H, W, 3)), _random_bytes(bufs.rng, (H, W))
    tiles = generate_tiles(W, H, (8, 16))
    odd = _clip([(3, 5, 41, 19), (47, 1, 29, 37), (1, 27, 45, 17)], W, H)
    covered = _mask(W, H, odd)
    rest = []  # the complement, as the runs of uncovered pixels of each row
    for y in range(H):
        x = 0
        while x < W:
            e = x
            while e < W and covered[y, e] == covered[y, x]:
                e += 1
            if not covered[y, x]:
                rest.append((x, y, e - x, 1))
            x = e
    try:
        for guided, levels in ((False, 3), (True, 3), (False, 5), (True, 0)):
            full_out, full_err = bufs.run(None, guided, out_init, err_init, levels=levels)
            for X, Y in ((tiles[::2], tiles[1::2]), (odd, rest)):
                for first, second in ((X, Y), (Y, X)):
                    bufs.run(first, guided, out_init, err_init, levels=levels)
                    bufs.call(second, guided, levels=levels)  # into the buffers as the first call left them
                    out, err = bufs.fbs[4].download(), bufs.err.download()
                    assert _bits(out).tobytes() == _bits(full_out).tobytes() and _bits(err).tobytes() == _bits(full_err).tobytes(), (guided, levels, len(first))
    finally:
        bufs.close()


def test_without_an_error_image_out_is_the_same_and_err_is_untouched(gpu_ctx):
    W, H = 70, 9
    bufs = _Buffers(gpu_ctx, W, H, 23)
    out_init, err_init = _random_bytes(bufs.rng, (H, W, 3)), _random_bytes(bufs.rng, (H, W))
    try:
        for guided in (False, True):
            for levels in (0, 3):
                full_out, _ = bufs.run(None, guided, out_init, err_init, levels=levels)
                for name, region in _region_sets(W, H, None).items():
                    out, err = bufs.run(region, guided, out_init, err_init, with_err=False, levels=levels)
                    assert _bits(out).tobytes() == _expect(_mask(W, H, region), full_out, out_init).tobytes(), (name, guided, levels)
                    assert err.tobytes() == err_init.tobytes(), (name, guided, levels)  # err_dev = NULL: the image the test holds was not the call's
    finally:
        bufs.close()


def test_the_scratch_grows_with_the_frame():
    """A context of its own, so that its first region call is the small one: 7 x 5, then 200 x 120 — which needs a larger block than the context holds —,
    then 7 x 5 again in the larger block."""
    with render.Context(0) as ctx:
        for W, H in ((7, 5), (200, 120), (7, 5)):
            bufs = _Buffers(ctx, W, H, 23)
            out_init, err_init = _random_bytes(bufs.rng, (H, W, 3)), _random_bytes(bufs.rng, (H, W))
            try:
                for guided in (False, True):
                    full_out, full_err = bufs.run(None, guided, out_init, err_init, levels=3)
                    region = _clip([(2, 1, 4, 3), (60, 40, 90, 31)], W, H)
                    mask = _mask(W, H, region)
                    out, err = bufs.run(region, guided, out_init, err_init, levels=3)
                    assert _bits(out).tobytes() == _expect(mask, full_out, out_init).tobytes(), (W, H, guided)
                    assert _bits(err).tobytes() == _expect(mask, full_err, err_init).tobytes(), (W, H, guided)
            finally:
                bufs.close()


def test_the_arrays_form_passes_the_region_and_the_initial_contents(gpu_ctx):
    W, H = 70, 9
    rng, halves, rects, counts_a, counts_b, F, G, counts_f = _inputs(W, H, 23)
    out_init, err_init = _random_bytes(rng, (H, W, 3)), _random_bytes(rng, (H, W))
    region = [(3, 2, 50, 5)]
    mask = _mask(W, H, region)
    for guide in ({}, dict(features=F, features_sq=G, counts_f=counts_f, **GUIDE)):
        full_out, full_err = render.denoise_atrous_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, levels=3, **guide)
        out, err = render.denoise_atrous_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, region=region, out_init=out_init, err_init=err_init, levels=3, **guide)
        assert _bits(out).tobytes() == _expect(mask, full_out, out_init).tobytes()
        assert _bits(err).tobytes() == _expect(mask, full_err, err_init).tobytes()


# ---------------------------------------------------------------- the adaptive render
SPP = 48  # passes of 8, no check below 16: checks at 16 and at 32 samples, the second over the tiles the first left live


def _settings(**kw):
    return Settings(scenes.camera(HW, HH), sample_count=SPP, tile_size=(32, 32), bounce_limit=HBOUNCES, seed=scenes.SEED, samples_per_iteration=HSPI, denoise=True,
                    denoise_dual=True, denoise_alpha=0.75, denoise_atrous_levels=4, denoise_atrous_k=2.5, denoise_feature_k=HGUIDE["k_f"],
                    denoise_feature_tau=HGUIDE["tau"], denoise_dual_atrous=True, adaptive_min_samples=16, **kw)


def _run_cli(tmp_path, which, tag, extra):
    cli = _cli()
    assert os.path.samefile(cli, CLI)
    ppm, raw = tmp_path / (tag + ".ppm"), tmp_path / (tag + ".f64")
    r = subprocess.run([cli, "render", "spheres" if which == "spheres" else "dragon:24", str(HW), str(HH), str(SPP), str(HBOUNCES), str(ppm), "--raw", str(raw), "--spi",
                        str(HSPI), *CLI_ARGS, "--adaptive-min", "16", *extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return ppm.read_bytes(), raw.read_bytes()


@pytest.mark.parametrize("which,guided", [("spheres", False), ("mesh", False), ("mesh", True)])
def test_the_adaptive_render_is_unchanged_and_uses_the_region_form(gpu_ctx, which, guided, monkeypatch, tmp_path):
    """The threshold is the median rmd_tile_error_dual the first check sees (a first run under a threshold nothing meets), so that some tiles finish
    there and the second check's live tiles are a proper part of the frame."""
    sc = _scene(which)
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
    more = dict(denoise_dual_features=guided)
    render.render_tiled(sc, _settings(adaptive_denoised_threshold=1e-300, **more), devices=(0,))
    threshold = float(np.median(calls[1][2]))
    del calls[:]
    off = render.render_tiled(sc, _settings(adaptive_denoised_threshold=threshold, **more), devices=(0,))
    calls_off = list(calls)
    del calls[:]
    on = render.render_tiled(sc, _settings(adaptive_denoised_threshold=threshold, denoise_dual_atrous_region=True, **more), devices=(0,))
    calls_on = list(calls)
    del calls[:]
    # two checks each; the second over a proper part of the frame
    assert [c[0] for c in calls_off] == [c[0] for c in calls_on] == ["filter", "error"] * 2
    live = [c[1] for c in calls_on if c[0] == "error"]
    assert live[0] == tiles and 0 < len(live[1]) < len(tiles) and set(live[1]) < set(tiles)
    print("adaptive a-trous region check (%s%s): threshold %.6g, live tiles at the checks %s" % (which, ", guided" if guided else "", threshold, [len(x) for x in live]))
    # on: region = the live tiles, while the rects describe the whole frame; off: no region keyword at all, the call made before the setting existed
    for (_, rects, kw), lv in zip([c for c in calls_on if c[0] == "filter"], live):
        assert kw["region"] == lv and sorted(rects) == sorted(tiles)
    assert all("region" not in c[2] for c in calls_off if c[0] == "filter")
    # the live tiles' errors are the same bits, and so are the messages — progress snapshots, finished tiles with their counts and errors
    assert [np.float64(c[2]).tobytes() for c in calls_on if c[0] == "error"] == [np.float64(c[2]).tobytes() for c in calls_off if c[0] == "error"]
    got, expected = [_message_key(m) for m in on._messages], [_message_key(m) for m in off._messages]
    assert len(got) == len(expected)
    for g, e in zip(got, expected):
        assert g == e, (g[:4], e[:4])
    fin, fin_off = tgd._finished_tiles(on), tgd._finished_tiles(off)  # (past the progress snapshots, as await_ needs them)
    assert [(t.left, t.top, t.sample_count, t.error) for t in fin] == [(t.left, t.top, t.sample_count, t.error) for t in fin_off]
    assert 2 * HSPI in {t.sample_count for t in fin} and max(t.sample_count for t in fin) > 2 * HSPI and any(t.error is not None for t in fin)
    # await_'s frame is the whole-frame call's either way
    frame_on, frame_off = on.await_(), off.await_()
    assert frame_on.tobytes() == frame_off.tobytes() and np.isfinite(frame_on).all()
    assert all(c[0] == "filter" and c[2].get("region") is None for c in calls) and len(calls) == 2
    monkeypatch.undo()
    # the C++ loop: identical files with and without the flag, the frame above, and the region entry point among the imports
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _cli()], check=True, capture_output=True, text=True).stdout
    assert "rmd_denoise_atrous_dual_region" in undefined.split()
    extra = ["--adaptive-denoised", "%.17g" % threshold] + (["--denoise-dual-features", "1"] if guided else [])
    without = _run_cli(tmp_path, which, "off", extra)
    with_flag = _run_cli(tmp_path, which, "on", extra + ["--denoise-dual-atrous-region", "1"])
    assert with_flag == without
    assert np.frombuffer(with_flag[1]).reshape(HH, HW, 3).tobytes() == frame_on.tobytes()
