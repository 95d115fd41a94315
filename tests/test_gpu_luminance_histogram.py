"""rmd_luminance_histogram_tiles on the GPU: all 262 integers against the numpy restatement (tests/luma_ref.py) — on frames of at most 67 x 45 whose
luminances lie ON the bin edges, next to them and on the specials, over rect lists that exercise the workgroup table, with and without a second sum
buffer, whatever the cuts, on a frame of one value — and settings.preview_auto_exposure through both render loops."""
import ctypes as C
import time

import numpy as np
import pytest

import luma_ref
from raymond_amd import abi, render, scenes
from raymond_amd.scene import Settings, generate_tiles, tile_array

pytestmark = pytest.mark.gpu

W, H = 67, 45
# a 40 x 30 rect (1,200 pixels: a chunk boundary inside a rect) followed by a 3 x 5 rect (a rect boundary inside a chunk), a rect without pixels, the rest
# of the frame, and two rects that overlap the others and each other; counts 0, 1, 7 and 4096
RECTS = [(0, 0, 40, 30), (40, 0, 3, 5), (50, 10, 0, 9), (43, 0, 24, 45), (0, 30, 43, 15), (40, 5, 3, 25), (10, 10, 20, 25), (25, 20, 30, 20)]
COUNTS = [1, 7, 4096, 4096, 7, 0, 1, 4096]


def upload(ctx, arr):
    fb = render.Framebuffer(ctx, arr.shape[1], arr.shape[0])
    fb.upload(arr)
    return fb


def device_histogram(ctx, acc, rects, counts, second=None):
    fbs = [upload(ctx, acc)] + ([upload(ctx, second)] if second is not None else [])
    try:
        return render.luminance_histogram(ctx, fbs[0], rects, counts, second=fbs[1] if second is not None else None)
    finally:
        for fb in fbs:
            fb.close()


def same(got, want, what=""):
    a, b = got.counters(), want.counters()
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, [(int(i), int(a[i]), int(b[i])) for i in bad[:12]])


@pytest.fixture(scope="module")
def edge_frame():
    """Sums whose means' luminances are the stand-alone program's values, scattered over the frame: every pixel's sum is made for the count of the FIRST
    rect that covers it.  Returns the sums and the set of target luminances."""
    rng = np.random.default_rng(21)
    targets = luma_ref.edge_values()
    radiances = [luma_ref.radiance_with_luminance(v) for v in targets] + [[float(s)] * 3 for s in luma_ref.special_values()]
    order = rng.permutation(W * H) % len(radiances)
    count_of = np.full((H, W), 1, dtype=np.int64)
    for (l, t, w, h), c in reversed(list(zip(RECTS, COUNTS))):
        count_of[t : t + h, l : l + w] = c
    acc = np.zeros((H, W, 3))
    for i, k in enumerate(order):
        y, x = divmod(i, W)
        acc[y, x] = [luma_ref.sum_for(p, int(count_of[y, x])) for p in radiances[k]]
    return acc, targets


def test_every_counter_exactly_on_edges_neighbours_and_specials(gpu_ctx, edge_frame):
    acc, targets = edge_frame
    ys = luma_ref.rect_luminances(acc, RECTS, COUNTS)
    hit = np.isin(np.array(targets), ys)
    print("targets that are some packed pixel's luminance, exactly: %d of %d" % (hit.sum(), hit.size))
    assert hit.all()  # the frame is what it is meant to be: every edge, and the doubles on either side of it
    want = luma_ref.histogram(acc, RECTS, COUNTS)
    assert want.pixels == sum(w * h for (_, _, w, h) in RECTS) and want.pixels > W * H  # (the overlaps are counted twice)
    assert min(want.zero, want.negative, want.not_finite, want.below, want.above) > 0 and np.count_nonzero(want.bins) == 256
    same(device_histogram(gpu_ctx, acc, RECTS, COUNTS), want)
    # the frame as one rect at every count, and a list that begins off a chunk's start
    for c in (1, 7, 4096, 0):
        same(device_histogram(gpu_ctx, acc, [(0, 0, W, H)], [c]), luma_ref.histogram(acc, [(0, 0, W, H)], [c]), c)
    shifted = [(3, 3, 1, 1)] + RECTS[::-1]
    same(device_histogram(gpu_ctx, acc, shifted, [7] + COUNTS[::-1]), luma_ref.histogram(acc, shifted, [7] + COUNTS[::-1]))


def random_sums(rng, shape):
    """Uniformly random exponents over more than the bins' range, every channel filled, a few negatives, zeros and non-finite values."""
    a = np.exp2(rng.uniform(-40, 40, shape)) * rng.uniform(1, 2, shape)
    r = rng.uniform(size=shape[:2])
    a[r < 0.02] *= -1.0
    a[(r >= 0.02) & (r < 0.04)] = 0.0
    a[(r >= 0.04) & (r < 0.05)] = np.inf
    a[(r >= 0.05) & (r < 0.06)] = np.nan
    return a


def test_two_sum_buffers_are_the_histogram_of_their_numpy_sum(gpu_ctx):
    rng = np.random.default_rng(22)
    a = random_sums(rng, (H, W, 3))
    with np.errstate(all="ignore"):
        b = a * rng.uniform(-1.5, 1.5, a.shape)  # (of a's size: the addition rounds, and cancels where the factor is near -1)
    want = luma_ref.histogram(a, RECTS, COUNTS, second=b)
    same(device_histogram(gpu_ctx, a, RECTS, COUNTS, second=b), want)
    with np.errstate(all="ignore"):
        same(want, luma_ref.histogram(np.add(a, b), RECTS, COUNTS))
    apart = render.add_histograms(luma_ref.histogram(a, RECTS, COUNTS), luma_ref.histogram(b, RECTS, COUNTS))
    assert apart.pixels == 2 * want.pixels and not np.array_equal(apart.bins, 2 * want.bins)  # binning a and b by themselves is something else


def test_cuts_do_not_matter(gpu_ctx):
    rng = np.random.default_rng(23)
    acc = random_sums(rng, (H, W, 3))
    whole = [(0, 0, W, H)]
    tiles = generate_tiles(W, H, (8, 8))
    ragged = []  # random disjoint rects that cover the frame: columns of random widths cut into pieces of random heights
    x = 0
    while x < W:
        w = int(min(rng.integers(1, 20), W - x))
        y = 0
        while y < H:
            h = int(min(rng.integers(1, 20), H - y))
            ragged.append((x, y, w, h))
            y += h
        x += w
    order = rng.permutation(len(ragged))
    ragged = [ragged[i] for i in order]
    assert sum(w * h for (_, _, w, h) in ragged) == W * H and len(ragged) > 12
    want = luma_ref.histogram(acc, whole, [3])
    fb = upload(gpu_ctx, acc)
    try:
        for rects in (whole, tiles, ragged):
            same(render.luminance_histogram(gpu_ctx, fb, rects, [3] * len(rects)), want, len(rects))
        # several devices: each over its own tiles, the integers added in either order
        parts = [render.luminance_histogram(gpu_ctx, fb, tiles[i::3], [3] * len(tiles[i::3])) for i in range(3)]
        same(render.add_histograms(render.add_histograms(parts[0], parts[1]), parts[2]), want)
        same(render.add_histograms(parts[2], render.add_histograms(parts[1], parts[0])), want)
    finally:
        fb.close()


def test_a_frame_of_one_value_lands_in_one_bin(gpu_ctx):
    """Every lane of every wave holds the same counter: the contention path."""
    acc = np.full((H, W, 3), 0.05 * 16)
    fb = upload(gpu_ctx, acc)
    try:
        t0 = time.perf_counter()
        got = render.luminance_histogram(gpu_ctx, fb, [(0, 0, W, H)], [16])
        seconds = time.perf_counter() - t0
    finally:
        fb.close()
    want = luma_ref.histogram(acc, [(0, 0, W, H)], [16])
    assert np.count_nonzero(want.bins) == 1 and int(want.bins.max()) == W * H == want.pixels
    same(got, want)
    print("one call on a constant %d x %d frame: %.3f ms" % (W, H, seconds * 1e3))
    assert seconds < 2.0  # (a synchronous call on 3,015 pixels: milliseconds, first launch included)


def test_no_rects_and_a_count_of_zero(gpu_ctx):
    fb = render.Framebuffer(gpu_ctx, W, H)
    try:
        fb.zero()
        out = abi.LumaHistogram()
        C.memset(C.byref(out), 0xAB, C.sizeof(out))
        assert gpu_ctx.L.rmd_luminance_histogram_tiles(gpu_ctx.handle, fb.ptr, None, W, H, None, None, 0, C.byref(out)) == abi.RMD_OK
        assert bytes(out) == bytes(C.sizeof(out))  # n_rects = 0: an all-zero histogram
        C.memset(C.byref(out), 0xAB, C.sizeof(out))
        empty = tile_array([(5, 5, 0, 3)])
        assert gpu_ctx.L.rmd_luminance_histogram_tiles(gpu_ctx.handle, fb.ptr, None, W, H, empty, (C.c_uint32 * 1)(4), 1, C.byref(out)) == abi.RMD_OK
        assert bytes(out) == bytes(C.sizeof(out))  # ... and rects without pixels
        got = render.luminance_histogram(gpu_ctx, fb, [(0, 0, W, H), (3, 3, 5, 5)], [0, 2])
        assert got.not_finite == W * H and got.zero == 25 and got.pixels == W * H + 25 and not got.bins.any()  # 0 / 0 is a NaN; 0 / 2 a zero
        # a refused call leaves the output alone and the context usable
        C.memset(C.byref(out), 0xAB, C.sizeof(out))
        outside = tile_array([(W - 3, 0, 4, 4)])
        status = gpu_ctx.L.rmd_luminance_histogram_tiles(gpu_ctx.handle, fb.ptr, None, W, H, outside, (C.c_uint32 * 1)(4), 1, C.byref(out))
        assert status == abi.RMD_ERR_INVALID_ARGUMENT and bytes(out) == b"\xab" * C.sizeof(out)
        assert b"rmd_luminance_histogram_tiles: tile rectangle outside the framebuffer" in gpu_ctx.L.rmd_last_error(gpu_ctx.handle)
        assert render.luminance_histogram(gpu_ctx, fb, [(0, 0, 2, 2)], [1]).zero == 4
    finally:
        fb.close()


def test_the_kept_scratch_grows_with_a_larger_second_call():
    rng = np.random.default_rng(24)
    acc = random_sums(rng, (H, W, 3))
    tiles = generate_tiles(W, H, (8, 8))
    with render.Context(0) as ctx:
        fb = upload(ctx, acc)
        try:
            same(render.luminance_histogram(ctx, fb, [(1, 1, 2, 2)], [1]), luma_ref.histogram(acc, [(1, 1, 2, 2)], [1]))
            same(render.luminance_histogram(ctx, fb, tiles, [5] * len(tiles)), luma_ref.histogram(acc, tiles, [5] * len(tiles)))
            same(render.luminance_histogram(ctx, fb, [(1, 1, 2, 2)], [1]), luma_ref.histogram(acc, [(1, 1, 2, 2)], [1]))
        finally:
            fb.close()


# ---------------------------------------------------------------- the render loops
RW, RH, SPP, SPI, BOUNCES = 64, 36, 12, 4, 4
TILES = generate_tiles(RW, RH, (32, 32))


def settings(**kw):
    return Settings(scenes.camera(RW, RH), sample_count=SPP, tile_size=(32, 32), bounce_limit=BOUNCES, samples_per_iteration=SPI, seed=scenes.SEED, **kw)


def run(st, devices=(0,)):
    handle = render.render_tiled(scenes.reflective_spheres(), st, devices)
    out = []
    while True:
        m = handle.poll()
        if m is None:
            return out
        out.append(m)


def previews(messages):
    return [m for m in messages if m.kind == "FramePreview"]


def sums_at(messages, sample_count):
    """The frame of sums a pass's TileProgressed messages carry."""
    acc = np.zeros((RH, RW, 3))
    tiles = [m.tile for m in messages if m.kind == "TileProgressed" and m.tile.sample_count == sample_count]
    assert len(tiles) == len(TILES)
    for t in tiles:
        acc[t.top : t.top + t.height, t.left : t.left + t.width] = t.data
    return acc


def check_preview(ctx, p, acc, counts, what):
    """p.exposure is the restatement's on the frame `acc` at `counts`, and p.frame is resolve_tonemap_tiles of it at that exposure."""
    want = luma_ref.exposure(luma_ref.histogram(acc, TILES, counts))
    print(what, "pass", p.pass_index, "exposure", p.exposure)
    assert p.exposure == want, (what, p.pass_index, p.exposure, want)
    fb = upload(ctx, acc)
    try:
        frame = render.scatter_tiles(TILES, render.resolve_tonemap_tiles(ctx, fb, TILES, counts, p.exposure, 2.2), RW, RH)
    finally:
        fb.close()
    assert np.array_equal(p.frame, frame), what


@pytest.mark.parametrize("devices", [(0,), (0, 0)])
def test_raw_previews_carry_the_exposure_of_that_passes_sums(gpu_ctx, devices):
    messages = run(settings(preview_every=1, preview_auto_exposure=True), devices)
    pv = previews(messages)
    assert [(p.pass_index, p.sample_count) for p in pv] == [(1, 4), (2, 8)]
    for p in pv:
        check_preview(gpu_ctx, p, sums_at(messages, p.sample_count), [p.sample_count] * len(TILES), "raw on %d" % len(devices))
    assert all(np.isfinite(p.exposure) and p.exposure > 0.0 for p in pv)
    if len(devices) == 1:
        off = run(settings(preview_every=1))
        assert [p.exposure for p in previews(off)] == [None, None]
        assert [m.kind for m in off] == [m.kind for m in messages]  # the setting changes no message but the previews' bytes and exposure
        other = previews(run(settings(preview_every=1, preview_auto_exposure=True, auto_exposure_percentile=0.5, auto_exposure_target=0.18)))
        want = luma_ref.exposure(luma_ref.histogram(sums_at(messages, 4), TILES, [4] * len(TILES)), 0.5, 0.18)
        assert other[0].exposure == want != pv[0].exposure


def test_dual_loop_previews_carry_the_exposure_of_both_halves_added(gpu_ctx):
    messages = run(settings(preview_every=1, preview_auto_exposure=True, denoise=True, denoise_dual=True))
    pv = previews(messages)
    assert [(p.pass_index, p.sample_count) for p in pv] == [(1, 4), (2, 8)]
    for p in pv:  # (a TileProgressed tile of this loop carries a + b, numpy's one rounded addition)
        check_preview(gpu_ctx, p, sums_at(messages, p.sample_count), [p.sample_count] * len(TILES), "dual")
    assert [p.exposure for p in previews(run(settings(preview_every=1, denoise=True, denoise_dual=True)))] == [None, None]


def test_filtered_previews_carry_the_exposure_of_the_filtered_means(gpu_ctx):
    st = settings(preview_every=2, preview_auto_exposure=True, preview_denoise=True, denoise_atrous_levels=3, denoise_atrous_k=2.0)
    (p,) = previews(run(st))
    assert (p.pass_index, p.sample_count) == (2, 8)
    (pd,) = previews(run(settings(preview_every=2, preview_auto_exposure=True, preview_denoise=True, denoise_atrous_levels=3, denoise_atrous_k=2.0, denoise=True,
                                   denoise_dual=True)))
    ds = render.DeviceScene(gpu_ctx, scenes.reflective_spheres())
    fbs = [render.Framebuffer(gpu_ctx, RW, RH) for _ in range(5)]
    try:
        # the single-buffer loop: rmd_denoise_atrous on the same samples rendered afresh (the bits do not depend on the split into passes)
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, TILES, fbs[0], 0, 8, framebuffer_sq=fbs[1])
        render.denoise_atrous(gpu_ctx, fbs[0], fbs[1], TILES, [8] * len(TILES), fbs[4], levels=3, k=2.0, alpha=st.denoise_alpha)
        check_preview(gpu_ctx, p, fbs[4].download(), [1] * len(TILES), "filtered")
        # the dual loop: pass 1 went to half A, pass 2 to half B
        for fb in fbs:
            fb.zero()
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, TILES, fbs[0], 0, 4, framebuffer_sq=fbs[1])
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, TILES, fbs[2], 4, 4, framebuffer_sq=fbs[3])
        render.denoise_atrous_dual(gpu_ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), TILES, [4] * len(TILES), [4] * len(TILES), fbs[4], None, levels=3,
                                   k=st.denoise_atrous_k, alpha=st.denoise_alpha)
        check_preview(gpu_ctx, pd, fbs[4].download(), [1] * len(TILES), "filtered, dual")
    finally:
        for o in fbs + [ds]:
            o.close()


# ---------------------------------------------------------------- the C++ mirror
@pytest.fixture(scope="module")
def cli(product_lib):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-s", "-C", os.path.join(root, "raymond_amd", "host")], check=True)
    return os.path.join(root, "raymond_amd", "host", "raymond_cli")


def read_ppm(path):
    with open(path, "rb") as f:
        assert f.readline() == b"P6\n" and f.readline() == b"%d %d\n" % (RW, RH) and f.readline() == b"255\n"
        return np.frombuffer(f.read(), dtype=np.uint8).reshape(RH, RW, 3)


@pytest.mark.parametrize("dual", [False, True])
def test_cli_auto_exposure_writes_the_python_previews_and_exposes_the_final_image(cli, tmp_path, oracle, dual):
    import subprocess

    extra, kw = (["--denoise", "1", "--denoise-dual", "1"], dict(denoise=True, denoise_dual=True)) if dual else ([], {})
    out, raw, prefix = tmp_path / "final.ppm", tmp_path / "final.f64", tmp_path / "pv"
    r = subprocess.run([cli, "render", "spheres", str(RW), str(RH), str(SPP), str(BOUNCES), str(out), "--spi", str(SPI), "--preview-every", "1", "--preview-prefix",
                        str(prefix), "--auto-exposure", "1", "--auto-exposure-percentile", "0.9", "--auto-exposure-target", "0.5", "--raw", str(raw)] + extra,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    pv = previews(run(settings(preview_every=1, preview_auto_exposure=True, auto_exposure_percentile=0.9, auto_exposure_target=0.5, **kw)))
    assert sorted(p.name for p in tmp_path.glob("pv_*.ppm")) == ["pv_0001.ppm", "pv_0002.ppm"] and len(pv) == 2
    for k, p in enumerate(pv):  # the mirror's previews are tone-mapped at the exposures Python's carry
        assert np.array_equal(read_ppm("%s_%04d.ppm" % (prefix, k + 1)), p.frame), k
    # the final image: the mirror bins the frame it has on the host with the header the kernel is built from; --raw holds that frame untouched
    image = np.fromfile(raw, dtype=np.float64).reshape(RH, RW, 3)
    exposure = luma_ref.exposure(luma_ref.histogram(image, [(0, 0, RW, RH)], [1]), 0.9, 0.5)
    assert "auto exposure: %.17g\n" % exposure in r.stdout, (exposure, r.stdout)
    assert np.array_equal(read_ppm(out), oracle.resolve_tonemap(image, 1, exposure, 2.2))
    plain = subprocess.run([cli, "render", "spheres", str(RW), str(RH), str(SPP), str(BOUNCES), str(tmp_path / "plain.ppm"), "--spi", str(SPI), "--raw",
                            str(tmp_path / "plain.f64")] + extra, capture_output=True, text=True)
    assert plain.returncode == 0 and "auto exposure" not in plain.stdout
    assert (tmp_path / "plain.f64").read_bytes() == raw.read_bytes()  # the flags change no radiance
    assert np.array_equal(read_ppm(tmp_path / "plain.ppm"), oracle.resolve_tonemap(image, 1, 1.0, 2.2))
