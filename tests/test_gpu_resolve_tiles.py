"""rmd_resolve_tonemap_tiles on the GPU: the output stage over tile rects, each at its own sample count, byte for byte the oracle's
restatement of TaskHandle::await's division + cli_old/src/main.rs:161-181 — on the frames of test_output_stage_is_byte_exact_on_adversarial_frames at
96 x 80 (radiances ON the truncation boundaries of every level, the specials, a mix that takes the per-pixel fix-up route), over tile lists and
adversarial rect shapes, with and without a second sum buffer; plus the rules for empty rects, n_rects = 0, refused arguments and the kept scratch."""
import ctypes as C

import numpy as np
import pytest

from raymond_amd import abi, render
from raymond_amd.scene import generate_tiles, tile_array

pytestmark = pytest.mark.gpu

W, H = 96, 80
CYCLE = (1, 2, 3, 7, 16, 500)
PAIRS = ((1.0, 2.2), (0.5, 1.8))
TILES = [t for i, t in enumerate(generate_tiles(W, H, (32, 32))) if i != 4]  # (a): one tile left out
SHAPES = [(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (13, 9, 7, 5), (0, 41, W, 1), (57, 0, 1, H), (20, 30, 0, 6),
          (0, 0, W, H)]  # (b): single pixels at the corners, a ragged rect, a row, a column, a rect without pixels, the whole frame
RECT_LISTS = {"tiles": TILES, "shapes": SHAPES}


def counts_for(rects, shift=0):
    return [CYCLE[(i + shift) % len(CYCLE)] for i in range(len(rects))]


@pytest.fixture(scope="module")
def frames():
    """Radiance frames (what acc / count * exposure should come to), made once."""
    rng = np.random.default_rng(5)
    levels = np.arange(1, 256, dtype=np.float64)
    with np.errstate(divide="ignore"):  # level 255: p = +inf, kept: an infinite radiance is one of the cases
        on_boundary = -np.log1p(-((levels / 255.0) ** 2.2))  # p with 255 * (1 - exp(-p))^(1/2.2) ~ level
    out = {}
    for spread in (0.0, 1e-14, 1e-8):
        p = on_boundary[rng.integers(0, 255, size=(H, W, 3))]
        out["boundary %g" % spread] = p * (1.0 + spread * rng.uniform(-1, 1, size=p.shape))
    special = np.array([0.0, -0.0, 1e-300, 1e-20, 2.0**-54, 2.0**-53, 36.0, 36.7368, 36.9, 37.0, 37.4299, 38.0, 39.9999, 40.0, 41.0, 700.0, 1e300,
                        np.inf, -np.inf, np.nan, -1.0, -1e-9, -700.0, -710.0, 5e-6, 5.1e-6, 5.2e-6])
    out["special"] = special[rng.integers(0, len(special), size=(H, W, 3))]
    mix = rng.uniform(0, 4, size=(H, W, 3))
    mix[rng.uniform(size=(H, W)) < 0.004] = on_boundary[7]  # a handful of flagged pixels: the per-pixel route
    out["mix"] = mix
    return out


def sums_for(frame, rects, counts, exposure):
    """Sums in which rect i holds frame * counts[i] / exposure — painted last rect first, so that where rects overlap the EARLIER one's count holds (the
    whole frame, last of the shapes, lies under all of them): every rect then sees, at its own count, radiances on the boundaries."""
    with np.errstate(invalid="ignore", over="ignore"):
        acc = frame * 1.0 / exposure
        for (l, t, w, h), c in reversed(list(zip(rects, counts))):
            acc[t : t + h, l : l + w] = frame[t : t + h, l : l + w] * c / exposure
    return acc


def packed_call(ctx, fb, rects, counts, exposure, gamma, out, second=None, width=W, height=H, rects_ptr=True, counts_ptr=True, fb_ptr=True):
    """The raw call: its status, and `out` (a uint8 array, or None for a NULL output) as the library left it."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    return ctx.L.rmd_resolve_tonemap_tiles(ctx.handle, fb.ptr if fb_ptr else None, second, width, height, tile_array(rects) if rects_ptr else None,
                                           counts.ctypes.data_as(C.POINTER(C.c_uint32)) if counts_ptr else None, len(rects), exposure, gamma,
                                           None if out is None else out.ctypes.data_as(C.c_void_p))


def check_against_oracle(oracle, acc, rects, counts, got, exposure, gamma, what):
    assert len(got) == len(rects)
    for (l, t, w, h), c, g in zip(rects, counts, got):
        assert g.shape == (h, w, 3)
        want = oracle.resolve_tonemap(acc[t : t + h, l : l + w], c, exposure, gamma)
        assert np.array_equal(g, want), (what, (l, t, w, h), c, int((g != want).sum()))


@pytest.mark.parametrize("which", sorted(RECT_LISTS))
def test_every_rect_is_the_oracles_bytes_at_its_own_count(gpu_ctx, oracle, frames, which):
    rects = RECT_LISTS[which]
    fb = render.Framebuffer(gpu_ctx, W, H)
    try:
        for k, (name, frame) in enumerate(sorted(frames.items())):
            for exposure, gamma in PAIRS:
                counts = counts_for(rects, k)
                acc = sums_for(frame, rects, counts, exposure)
                fb.upload(acc)
                got = render.resolve_tonemap_tiles(gpu_ctx, fb, rects, counts, exposure, gamma)
                check_against_oracle(oracle, acc, rects, counts, got, exposure, gamma, (name, exposure, gamma))
    finally:
        fb.close()


def test_the_whole_frame_as_one_rect_is_rmd_resolve_tonemap(gpu_ctx, frames):
    fb = render.Framebuffer(gpu_ctx, W, H)
    try:
        for name, frame in sorted(frames.items()):
            for (exposure, gamma), spp in zip(PAIRS, (16, 7)):
                with np.errstate(invalid="ignore", over="ignore"):
                    fb.upload(frame * spp / exposure)
                whole = render.resolve_tonemap(gpu_ctx, fb, spp, exposure, gamma)
                (tile,) = render.resolve_tonemap_tiles(gpu_ctx, fb, [(0, 0, W, H)], [spp], exposure, gamma)
                assert np.array_equal(tile, whole), (name, spp, int((tile != whole).sum()))
    finally:
        fb.close()


@pytest.mark.parametrize("which", sorted(RECT_LISTS))
def test_two_sum_buffers_give_the_bytes_of_their_numpy_sum(gpu_ctx, oracle, frames, which):
    """accum2_dev: a frame split at random into two addends — the device adds them in one rounded addition, as numpy's a + b does."""
    rng = np.random.default_rng(11)
    rects = RECT_LISTS[which]
    fb_a, fb_b = render.Framebuffer(gpu_ctx, W, H), render.Framebuffer(gpu_ctx, W, H)
    try:
        for k, (name, frame) in enumerate(sorted(frames.items())):
            exposure, gamma = PAIRS[k % 2]
            counts = counts_for(rects, k + 1)
            with np.errstate(invalid="ignore", over="ignore"):
                acc = sums_for(frame, rects, counts, exposure)
                a = acc * rng.uniform(0.0, 1.0, size=acc.shape)
                a[~np.isfinite(a)] = 0.0
                b = acc - a  # a + b lands on or next to acc: still at the boundaries, and the check below is against a + b itself
                total = a + b
            fb_a.upload(a), fb_b.upload(b)
            got = render.resolve_tonemap_tiles(gpu_ctx, fb_a, rects, counts, exposure, gamma, second=fb_b)
            check_against_oracle(oracle, total, rects, counts, got, exposure, gamma, name)
    finally:
        fb_a.close(), fb_b.close()


def test_count_zero_over_zero_sums_is_black_and_an_empty_rect_shifts_nothing(gpu_ctx, oracle, frames):
    fb = render.Framebuffer(gpu_ctx, W, H)
    try:
        acc = frames["mix"] * 3.0
        acc[8:24, 40:72] = 0.0
        fb.upload(acc)
        rects = [(5, 5, 9, 4), (40, 8, 32, 16), (60, 60, 20, 11)]
        counts = [3, 0, 3]
        got = render.resolve_tonemap_tiles(gpu_ctx, fb, rects, counts)
        assert got[1].shape == (16, 32, 3) and not got[1].any()  # 0 / 0: the pixel stays (0, 0, 0)
        check_against_oracle(oracle, acc, [rects[0], rects[2]], [3, 3], [got[0], got[2]], 1.0, 2.2, "beside the count-0 rect")
        # the same list with rects without pixels in front, between and behind: the other rects' bytes are where they were
        holes = [(7, 7, 0, 5), rects[0], (30, 30, 4, 0), (0, 0, 0, 0), rects[1], rects[2], (95, 79, 0, 1)]
        got2 = render.resolve_tonemap_tiles(gpu_ctx, fb, holes, [9, 3, 9, 9, 0, 3, 9])
        assert [g.size for g in got2] == [0, 9 * 4 * 3, 0, 0, 32 * 16 * 3, 20 * 11 * 3, 0]
        for i, j in ((0, 1), (1, 4), (2, 5)):
            assert np.array_equal(got[i], got2[j])
    finally:
        fb.close()


def test_no_rects_and_refused_calls_leave_the_output_untouched(gpu_ctx, frames):
    fb, other = render.Framebuffer(gpu_ctx, W, H), render.Framebuffer(gpu_ctx, W, H)
    try:
        fb.upload(frames["mix"])
        out = np.full(W * H * 3, 0xAB, dtype=np.uint8)
        ok = [(0, 0, 32, 32), (32, 0, 32, 32)]
        assert packed_call(gpu_ctx, fb, [], [], 1.0, 2.2, out) == abi.RMD_OK and (out == 0xAB).all()  # n_rects = 0
        assert packed_call(gpu_ctx, fb, [], [], 1.0, 2.2, out, rects_ptr=False, counts_ptr=False) == abi.RMD_OK and (out == 0xAB).all()
        assert packed_call(gpu_ctx, fb, [(3, 3, 0, 9)], [4], 1.0, 2.2, None) == abi.RMD_OK  # rects without pixels need no output
        invalid = abi.RMD_ERR_INVALID_ARGUMENT
        inside = C.c_void_p(fb.ptr.value + 8 * 3 * W * (H // 2))  # half a frame further: overlaps accum_dev
        refused = {
            "accum_dev NULL": dict(fb_ptr=False),
            "width 0": dict(width=0),
            "height 0": dict(height=0),
            "rects NULL": dict(rects_ptr=False),
            "counts NULL": dict(counts_ptr=False),
            "rect past the right edge": dict(rects=[ok[0], (W - 31, 0, 32, 32)]),
            "rect past the lower edge": dict(rects=[ok[0], (0, H - 31, 32, 32)]),
            "rect whose left + width wraps": dict(rects=[(2**32 - 16, 0, 32, 32), ok[1]]),
            "accum2_dev is accum_dev": dict(second=fb.ptr),
            "accum2_dev overlaps accum_dev": dict(second=inside),
        }
        for what, kw in refused.items():
            rects = kw.pop("rects", ok)
            assert packed_call(gpu_ctx, fb, rects, [2] * len(rects), 1.0, 2.2, out, **kw) == invalid, what
            assert (out == 0xAB).all(), what
            assert b"rmd_resolve_tonemap_tiles" in gpu_ctx.L.rmd_last_error(gpu_ctx.handle), what
        assert packed_call(gpu_ctx, fb, ok, [2, 2], 1.0, 2.2, None) == invalid  # out NULL while the rects hold pixels
        # more than 2^32 - 1 packed pixels: a frame description large enough, never touched (the call is refused before the device is)
        big = 70000
        assert packed_call(gpu_ctx, fb, [(0, 0, big, big)], [1], 1.0, 2.2, out, width=big, height=big) == abi.RMD_ERR_UNSUPPORTED and (out == 0xAB).all()
        # ... and a second buffer that does not overlap is accepted after all that
        got = render.resolve_tonemap_tiles(gpu_ctx, fb, ok, [2, 2], second=other)
        assert np.array_equal(got[0], render.resolve_tonemap_tiles(gpu_ctx, fb, ok, [2, 2])[0])  # (other holds zeros)
    finally:
        fb.close(), other.close()


def test_the_kept_scratch_grows_with_a_larger_second_call(frames):
    """A small call, then a larger one on the same context: the larger one's bytes are a fresh context's."""
    acc = frames["mix"] * 16.0
    big = generate_tiles(W, H, (32, 32)) + SHAPES
    counts = counts_for(big)

    def on(ctx, rects, cnt):
        fb = render.Framebuffer(ctx, W, H)
        try:
            fb.upload(acc)
            return [g.copy() for g in render.resolve_tonemap_tiles(ctx, fb, rects, cnt)]
        finally:
            fb.close()

    with render.Context(0) as fresh:
        want = on(fresh, big, counts)
    with render.Context(0) as ctx:
        small = on(ctx, [(13, 9, 7, 5)], [16])
        got = on(ctx, big, counts)
        again = on(ctx, [(13, 9, 7, 5)], [16])  # ... and a smaller one after it reuses the block
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and np.array_equal(small[0], again[0])
