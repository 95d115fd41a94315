"""rmd_denoise_dual_region on the device: inside the region the bytes of rmd_denoise_dual, outside it nothing written; disjoint calls compose to the
whole frame; and the adaptive dual-buffer render (Python and raymond_cli) checks its live tiles through the region form and sends what it sent
when every check filtered the whole frame.

No tolerance anywhere: every comparison is tobytes() equality between two device results.  Frames, inputs and parameters are test_gpu_denoise's and
test_gpu_denoise_dual's own (imported from them)."""
import os
import subprocess

import numpy as np
import pytest

from raymond_amd import render, scenes
from raymond_amd.scene import generate_tiles
from test_gpu_denoise import CASES, _finished_tiles
from test_gpu_denoise_dual import CLI, _assemble_dual, _cli, _dual_settings, _two_halves

FRAMES = [(1, 1), (5, 200), (37, 23), (64, 48), (200, 120)]


def _clip(rects, W, H):
    """The parts of `rects` inside the frame (rects without pixels dropped)."""
    out = []
    for (l, t, w, h) in rects:
        w, h = min(l + w, W) - l, min(t + h, H) - t
        if w > 0 and h > 0:
            out.append((l, t, w, h))
    return out


def _region_sets(W, H):
    corners = sorted({(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1)})
    return {"whole_frame": [(0, 0, W, H)],
            "every_other_8x16_tile": generate_tiles(W, H, (8, 16))[::2],
            "corners": corners,
            # aligned to neither 16 nor the kernel's tile width (32 or 24), wider and higher than one workgroup's tile, pairwise disjoint
            "unaligned": _clip([(3, 5, 41, 19), (47, 1, 29, 37), (1, 27, 45, 17), (101, 33, 77, 55)], W, H),
            "empty": []}


def _mask(W, H, region):
    m = np.zeros((H, W), dtype=bool)
    for (l, t, w, h) in region:
        assert not m[t : t + h, l : l + w].any(), "the test's own region overlaps itself"
        m[t : t + h, l : l + w] = True
    return m


def _random_bytes(rng, shape):
    """Doubles of random BYTES (NaNs of every payload among them): whatever is not written must come back bit for bit."""
    return rng.integers(0, 256, int(np.prod(shape)) * 8, dtype=np.uint8).view(np.float64).reshape(shape).copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class _Buffers:
    """The two halves uploaded once; out and err re-filled before each call."""

    def __init__(self, ctx, halves):
        self.ctx = ctx
        H, W = halves[0].shape[:2]
        self.fbs = [render.Framebuffer(ctx, W, H) for _ in range(5)]
        self.err = render.ErrorImage(ctx, W, H)
        for fb, arr in zip(self.fbs, halves):
            fb.upload(arr)

    def run(self, rects, counts_a, counts_b, region, out_init, err_init, with_err=True, **params):
        self.fbs[4].upload(out_init), self.err.upload(err_init)
        render.denoise_dual(self.ctx, (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3]), rects, counts_a, counts_b, self.fbs[4],
                            self.err if with_err else None, region=region, **params)
        return self.fbs[4].download(), self.err.download()

    def again(self, rects, counts_a, counts_b, region, **params):
        """A further call into the buffers as the last one left them."""
        render.denoise_dual(self.ctx, (self.fbs[0], self.fbs[1]), (self.fbs[2], self.fbs[3]), rects, counts_a, counts_b, self.fbs[4], self.err, region=region, **params)
        return self.fbs[4].download(), self.err.download()

    def close(self):
        for b in self.fbs + [self.err]:
            b.close()


def _inputs(W, H):
    rng = np.random.default_rng(W * 1000 + H + 11)
    halves, rects, counts_a, counts_b, _, _ = _two_halves(rng, W, H)  # poisoned sums, counts of 0 and 1, one tile uncovered
    return rng, halves, rects, counts_a, counts_b


def _expect(mask, full, init):
    return np.where(mask if full.ndim == 2 else mask[..., None], _bits(full), _bits(init))


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", FRAMES)
def test_region_equals_the_full_frame_and_nothing_else_is_written(gpu_ctx, W, H):
    rng, halves, rects, counts_a, counts_b = _inputs(W, H)
    out_init, err_init = _random_bytes(rng, (H, W, 3)), _random_bytes(rng, (H, W))
    bufs = _Buffers(gpu_ctx, halves)
    try:
        for r, f, k, alpha in CASES:
            params = dict(radius=r, patch_radius=f, k=k, alpha=alpha)
            full_out, full_err = bufs.run(rects, counts_a, counts_b, None, out_init, err_init, **params)
            for name, region in _region_sets(W, H).items():
                mask = _mask(W, H, region)
                out, err = bufs.run(rects, counts_a, counts_b, region, out_init, err_init, **params)
                assert _bits(out).tobytes() == _expect(mask, full_out, out_init).tobytes(), (name, params)
                assert _bits(err).tobytes() == _expect(mask, full_err, err_init).tobytes(), (name, params)
        # (the inputs make the comparison mean something: dual-valid pixels and others, inside the frame's regions)
        assert W * H == 1 or (np.isnan(full_err).any() and np.isfinite(full_err).any())  # (the 1 x 1 frame is one dual-valid pixel)
    finally:
        bufs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(37, 23), (200, 120)])
def test_two_disjoint_calls_compose_to_the_full_frame_in_both_orders(gpu_ctx, W, H):
    rng, halves, rects, counts_a, counts_b = _inputs(W, H)
    out_init, err_init = _random_bytes(rng, (H, W, 3)), _random_bytes(rng, (H, W))
    tiles = generate_tiles(W, H, (8, 16))
    # a set and its complement: every other tile and the rest; three odd rects and the rest of the frame cut around them
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
    bufs = _Buffers(gpu_ctx, halves)
    try:
        for r, f, k, alpha in (CASES[3], CASES[4], CASES[1]):
            params = dict(radius=r, patch_radius=f, k=k, alpha=alpha)
            full_out, full_err = bufs.run(rects, counts_a, counts_b, None, out_init, err_init, **params)
            for X, Y in ((tiles[::2], tiles[1::2]), (odd, rest)):
                for first, second in ((X, Y), (Y, X)):
                    bufs.run(rects, counts_a, counts_b, first, out_init, err_init, **params)
                    out, err = bufs.again(rects, counts_a, counts_b, second, **params)
                    assert out.tobytes() == full_out.tobytes() and err.tobytes() == full_err.tobytes(), (params, len(first), len(second))
    finally:
        bufs.close()


@pytest.mark.gpu
def test_without_an_error_image_out_is_the_same_and_err_is_untouched(gpu_ctx):
    W, H = 64, 48
    rng, halves, rects, counts_a, counts_b = _inputs(W, H)
    out_init, err_init = _random_bytes(rng, (H, W, 3)), _random_bytes(rng, (H, W))
    bufs = _Buffers(gpu_ctx, halves)
    try:
        for r, f, k, alpha in CASES:
            params = dict(radius=r, patch_radius=f, k=k, alpha=alpha)
            full_out, _ = bufs.run(rects, counts_a, counts_b, None, out_init, err_init, **params)
            for name, region in _region_sets(W, H).items():
                out, err = bufs.run(rects, counts_a, counts_b, region, out_init, err_init, with_err=False, **params)
                assert _bits(out).tobytes() == _expect(_mask(W, H, region), full_out, out_init).tobytes(), (name, params)
                assert err.tobytes() == err_init.tobytes(), (name, params)  # err_dev = NULL: the image the test holds was not the call's
    finally:
        bufs.close()


@pytest.mark.gpu
def test_the_arrays_form_passes_the_initial_contents(gpu_ctx):
    """render.denoise_dual_arrays(region=, out_init=, err_init=): the public way to see the 'not written' rule."""
    W, H = 37, 23
    rng, halves, rects, counts_a, counts_b = _inputs(W, H)
    out_init, err_init = _random_bytes(rng, (H, W, 3)), _random_bytes(rng, (H, W))
    region = [(3, 5, 30, 11)]
    full_out, full_err = render.denoise_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, radius=3, patch_radius=1)
    out, err = render.denoise_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, region=region, out_init=out_init, err_init=err_init, radius=3, patch_radius=1)
    mask = _mask(W, H, region)
    assert _bits(out).tobytes() == _expect(mask, full_out, out_init).tobytes()
    assert _bits(err).tobytes() == _expect(mask, full_err, err_init).tobytes()


# ---------------------------------------------------------------- the adaptive render
def _parent_policy(ctx, scene, st):
    """The adaptive dual-buffer loop as it was before the region form, restated: after every even number of passes that leaves live tiles below
    sample_count with at least adaptive_min_samples, the WHOLE-FRAME render.denoise_dual and render.tile_error_dual over the live tiles; whole
    framebuffers downloaded.  -> (messages as (kind, rect, count, error, data bytes ...) tuples, the live tiles at each check)."""
    cam = st.camera_settings
    W, H = cam.backbuffer_width, cam.backbuffer_height
    params = dict(radius=st.denoise_radius, patch_radius=st.denoise_patch, k=st.denoise_k, alpha=st.denoise_alpha)
    ds = render.DeviceScene(ctx, scene)
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(5)]
    err_img = render.ErrorImage(ctx, W, H)
    progressed, finished, checks = [], [], []
    try:
        live = generate_tiles(W, H, st.tile_size)
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
            done, j = done + n, j + 1
            n_half[half] += n
            if done < st.sample_count:
                errors = [None] * len(live)
                if j % 2 == 0 and done >= st.adaptive_min_samples:
                    checks.append(list(live))
                    render.denoise_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), done_rects + live, done_a + [n_half[0]] * len(live),
                                        done_b + [n_half[1]] * len(live), fbs[4], err_img, **params)
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
        for o in fbs + [err_img, ds]:
            o.close()
    return progressed + finished, checks


def _key(kind, rect, count, error, *rest):
    """A message as plain values: the error by its bits, every array by its shape and bytes."""
    return (kind, tuple(rect), count, None if error is None else np.float64(error).tobytes(),
            tuple(x if x is None or isinstance(x, int) else (x.shape, np.ascontiguousarray(x).tobytes()) for x in rest))


def _message_key(m):
    t = m.tile
    rect = (t.left, t.top, t.width, t.height)
    if m.kind == "TileProgressed":
        assert t.data_sq is None and t.data_a is None and t.count_a is None
        return _key(m.kind, rect, t.sample_count, t.error, t.data)
    return _key(m.kind, rect, t.sample_count, t.error, t.data, t.data_sq, t.data_a, t.data_sq_a, t.data_b, t.data_sq_b, t.count_a, t.count_b)


def _quantile_threshold(ctx, W, H, bounces, **params):
    """The threshold of test_render_tiled_dual_equals_rmd_denoise_dual_over_the_tiles[adaptive]: the MEDIAN rmd_tile_error_dual of the 32x32 tiles
    of a uniform 6 spp dual render (passes of 3) — _median_dual_tile_error's value, computed here with the tile errors kept for the report."""
    handle = render.render_tiled(scenes.reflective_spheres(), _dual_settings(W, H, 6, 3, bounces), devices=(0,))
    halves, rects, counts_a, counts_b = _assemble_dual(_finished_tiles(handle), W, H)
    fbs = [render.Framebuffer(ctx, W, H) for _ in range(5)]
    err = render.ErrorImage(ctx, W, H)
    try:
        for fb, arr in zip(fbs, halves):
            fb.upload(arr)
        render.denoise_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), rects, counts_a, counts_b, fbs[4], err, **params)
        errors = render.tile_error_dual(ctx, err, rects)
    finally:
        for fb in fbs + [err]:
            fb.close()
    print("tile errors at 6 spp:", sorted(float(e) for e in errors), "median", float(np.median(errors)))
    return float(np.median(errors))


@pytest.mark.gpu
def test_the_adaptive_render_is_unchanged_and_uses_the_region_form(gpu_ctx, monkeypatch, tmp_path):
    """ReflectiveSpheres 96x64, 4 bounces, 32x32 tiles, passes of 3, no check below 6 samples, r = 5, f = 2 — the scene, size and threshold (the
    median tile error at 6 spp) of test_render_tiled_dual_equals_rmd_denoise_dual_over_the_tiles[adaptive] — with sample_count 18 instead of 12, so
    that there are two checks (at 6 and at 12 samples) and the second one's live tiles are a proper part of the frame.  The median splits the tiles:
    some finish at a check, others reach sample_count (asserted below).  (The CPU oracle's frames through the numpy restatement: tile errors
    0.026 - 0.029 and 0.051 - 0.069 at 6 samples, median 0.0398, so three tiles finish there; 0.030, 0.041 and 0.045 for the other three at 12, so one
    more finishes and two go on to 18.)"""
    W, H, bounces, spp, spi = 96, 64, 4, 18, 3
    sc = scenes.reflective_spheres()
    params = dict(radius=5, patch_radius=2, k=0.45, alpha=1.0)
    threshold = _quantile_threshold(gpu_ctx, W, H, bounces, **params)
    st = _dual_settings(W, H, spp, spi, bounces, denoise_radius=5, denoise_patch=2, adaptive_denoised_threshold=threshold, adaptive_min_samples=6)
    expected, checks = _parent_policy(gpu_ctx, sc, st)
    all_tiles = generate_tiles(W, H, (32, 32))
    counts = [m[2] for m in expected if m[0] == "TileFinished"]
    print("checks over", [len(c) for c in checks], "live tiles; finished at", sorted(counts))
    assert min(counts) < spp, "no tile finished at a check"
    assert max(counts) == spp, "no tile went on to sample_count"
    assert len(checks) >= 2 and 0 < len(checks[-1]) < len(all_tiles), "no check over a proper part of the frame"

    calls = []
    real = render.denoise_dual

    def spy(ctx, half_a, half_b, rects, counts_a, counts_b, out_framebuffer, error_image=None, region=None, **kw):
        calls.append((None if region is None else list(region), list(rects)))
        return real(ctx, half_a, half_b, rects, counts_a, counts_b, out_framebuffer, error_image, region=region, **kw)

    monkeypatch.setattr(render, "denoise_dual", spy)
    handle = render.render_tiled(sc, st, devices=(0,))
    in_loop = list(calls)
    monkeypatch.setattr(render, "denoise_dual", real)
    assert [r for r, _ in in_loop] == checks  # each check's region was exactly the live tiles; no whole-frame call (region None) inside the loop
    assert all(sorted(rects) == sorted(all_tiles) for _, rects in in_loop)  # while the rects still describe the whole frame
    got = [_message_key(m) for m in handle._messages]
    assert len(got) == len(expected)
    for g, e in zip(got, expected):
        assert g == e, (g[:4], e[:4])
    # await_'s frame stays the whole-frame rmd_denoise_dual over the finished tiles
    tiles = _finished_tiles(handle)
    halves, rects, counts_a, counts_b = _assemble_dual(tiles, W, H)
    frame, _ = render.denoise_dual_arrays(gpu_ctx, *halves, rects, counts_a, counts_b, **params)
    img_py = handle.await_()
    assert img_py.tobytes() == frame.tobytes()

    # the C++ mirror: raymond_cli calls the region form, and its frame is the same bytes
    cli = _cli()
    undefined = subprocess.run(["nm", "-D", "--undefined-only", cli], check=True, capture_output=True, text=True).stdout
    assert "rmd_denoise_dual_region" in undefined
    ppm, raw = tmp_path / "o.ppm", tmp_path / "o.f64"
    r = subprocess.run([cli, "render", "spheres", str(W), str(H), str(spp), str(bounces), str(ppm), "--raw", str(raw), "--spi", str(spi), "--denoise", "1",
                        "--denoise-dual", "1", "--denoise-radius", "5", "--denoise-patch", "2", "--adaptive-denoised", "%.17g" % threshold, "--adaptive-min", "6"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert np.fromfile(raw).reshape(H, W, 3).tobytes() == frame.tobytes()
    assert os.path.samefile(cli, CLI)
