"""rmd_tile_error and rmd_tile_error_dual on the GPU against their restatements (tests/tile_error_ref.py) on the frames of tests/tile_error_frames.py, which
tests/test_tile_error_host.py holds to what they name.

rmd_tile_error: one call with every pixel as a 1 x 1 rect gives the device's own per-pixel map D.  D follows pixel_errors — +inf and 0 exactly, no NaN, else
within the 1e-12 relative that tests/test_gpu_tile_luma.py and tests/test_gpu_despike.py hold this kernel's root to —, and every rect's result is D's maximum
over the rect BIT FOR BIT: a maximum has no order, so any difference is a fault of the lane, wave or shared-memory reduction.  A planted worst pixel at each
end of each wave; the sample counts 0, 1, 2^24 + 1 and 2^32 - 1; the call shapes and refusals.

rmd_tile_error_dual: err images of the test's own, uploaded through render.ErrorImage.  Only the last division and the root separate the device from the
restated total, so 1e-12 relative holds the header's sum order: on `chain` and `pairs` every other order is more than 1e-3 away.  Totals whose mean is an exact
square give exact results; the position of a rect and the frame's width change no bit.

And the decision at equality: with a tile's own error as the threshold the tile finishes at that check, with the next double below it does not — through
render_tiled and through raymond_cli."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_gpu_moments as moments
import tile_error_frames as frames
import tile_error_ref as ref
from raymond_amd import abi, render, scenes
from raymond_amd.scene import Settings, tile_array

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [c.name for c in frames.cases()]


def assert_follows(got, want, what):
    """+inf and 0 exact, no NaN, else within 1e-12 relative; prints the largest relative and ulp distance."""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape, what
    assert not np.isnan(got).any(), (what, got)
    special = ~np.isfinite(want) | (want == 0.0)
    assert ref.same_bits(got[special], want[special]), (what, got[special], want[special])
    g, w = got[~special], want[~special]
    assert np.isfinite(g).all() and (g > 0).all(), (what, g)
    rel = np.abs(g - w) / w
    print("%-32s largest relative difference %.3g, largest ulp distance %d, over %d values" %
          (what, rel.max() if rel.size else 0.0, ref.ulp_distance(g, w).max() if g.size else 0, g.size))
    assert (rel <= 1e-12).all(), (what, g[rel > 1e-12], w[rel > 1e-12])


def pixel_rects(width, height):
    return [(x, y, 1, 1) for y in range(height) for x in range(width)]


class Device:
    """Two framebuffers of one size and what the device made of each case: name -> (D, the results of the case's rect list)."""

    def __init__(self, ctx, width, height):
        self.ctx, self.width, self.height = ctx, width, height
        self.fb, self.fb_sq = render.Framebuffer(ctx, width, height), render.Framebuffer(ctx, width, height)
        self.pixels = pixel_rects(width, height)
        self.made = {}

    def errors(self, S, Q, n, floor, rects):
        self.fb.upload(S), self.fb_sq.upload(Q)
        return render.tile_error(self.ctx, self.fb, self.fb_sq, n, floor, rects)

    def pixel_map(self, S, Q, n, floor):
        return self.errors(S, Q, n, floor, self.pixels).reshape(self.height, self.width)

    def run(self, c, rects):
        if c.name not in self.made:
            self.made[c.name] = (self.pixel_map(c.S, c.Q, c.n, c.floor), self.errors(c.S, c.Q, c.n, c.floor, rects))
        return self.made[c.name]

    def close(self):
        self.fb.close(), self.fb_sq.close()


@pytest.fixture(scope="module")
def small(gpu_ctx):
    d = Device(gpu_ctx, frames.W, frames.H)
    yield d
    d.close()


# ---------------------------------------------------------------- rmd_tile_error
@pytest.mark.parametrize("name", CASES)
def test_the_pixel_map_follows_the_restatement(small, name):
    c = frames.case(name)
    D, _ = small.run(c, frames.case_rects(c))
    want = ref.pixel_errors(c.S, c.Q, c.n, c.floor)
    assert_follows(D, want, name)
    if c.n < 2:
        assert (D == np.inf).all()


@pytest.mark.parametrize("name", CASES)
def test_every_rect_is_the_maximum_of_the_devices_own_pixel_map(small, name):
    c = frames.case(name)
    rects = frames.case_rects(c)
    D, got = small.run(c, rects)
    assert ref.same_bits(got, ref.rect_maxima(D, rects)), (name, got, ref.rect_maxima(D, rects))
    assert_follows(got, ref.tile_error(c.S, c.Q, c.n, c.floor, rects), name + " rects")
    with_pixels = np.array([r[2] * r[3] > 0 for r in rects])
    assert (got[~with_pixels] == 0.0).all()
    if c.n < 2:
        assert (got[with_pixels] == np.inf).all()
    if name.startswith("specials"):
        assert (got[:3] == np.inf).all()


def test_the_wide_frame_long_rects_and_the_whole_frame(gpu_ctx):
    c = frames.wide_case()
    d = Device(gpu_ctx, frames.WIDE, frames.WIDE)
    try:
        D, got = d.run(c, frames.WIDE_RECTS)
    finally:
        d.close()
    assert_follows(D, ref.pixel_errors(c.S, c.Q, c.n, c.floor), c.name)
    assert ref.same_bits(got, ref.rect_maxima(D, frames.WIDE_RECTS)), (got, ref.rect_maxima(D, frames.WIDE_RECTS))


@pytest.mark.parametrize("rect", frames.PLANT_RECTS)
def test_a_planted_worst_pixel_is_found_at_every_lane_and_trip(small, rect):
    q = frames.case("quiet")
    quiet = small.errors(q.S, q.Q, q.n, q.floor, [rect])[0]
    assert 0.0 < quiet < 0.0054
    for index in frames.PLANT_INDICES:
        x, y = frames.pixel_of(rect, index)
        got = small.errors(*frames.planted(q.S, q.Q, rect, index), q.n, q.floor, [rect, (x, y, 1, 1)])
        assert ref.same_bits(got[:1], got[1:]), (rect, index, got)
        assert got[0] >= 2.0 * quiet, (rect, index, got, quiet)
        assert abs(got[0] - 1.0) <= 1e-12  # Q = S^2 at 8 samples: v / n = m^2


def raw_tile_error(ctx, fb, fb_sq, n, floor, rects, n_rects, out):
    return ctx.L.rmd_tile_error(ctx.handle, fb.ptr, fb_sq.ptr, fb.width, fb.height, n, floor, tile_array(rects), n_rects, out.ctypes.data_as(C.c_void_p))


def test_call_shapes_and_refusals(small):
    c = frames.case("random/n=64")
    _, whole = small.run(c, frames.RECTS)
    ctx, fb, fb_sq = small.ctx, small.fb, small.fb_sq
    fb.upload(c.S), fb_sq.upload(c.Q)
    sentinel = np.full(4, -123.25)
    # no rects: RMD_OK, and the output array is as it was
    out = sentinel.copy()
    assert raw_tile_error(ctx, fb, fb_sq, c.n, c.floor, [], 0, out) == abi.RMD_OK
    assert out.tobytes() == sentinel.tobytes()
    # past the right edge, past the lower edge, left + width wrapping 32 bits: refused on the host, nothing written, the context good for the next call
    for bad in ((frames.W - 3, 0, 4, 1), (0, frames.H - 3, 1, 4), (2**32 - 1, 0, 2, 1), (0, 2**32 - 1, 1, 2)):
        for rects in ([bad], [frames.TILE, bad], [bad, frames.TILE]):
            out = sentinel.copy()
            assert raw_tile_error(ctx, fb, fb_sq, c.n, c.floor, rects, len(rects), out) == abi.RMD_ERR_INVALID_ARGUMENT, (bad, rects)
            assert out.tobytes() == sentinel.tobytes(), (bad, rects)
        again = render.tile_error(ctx, fb, fb_sq, c.n, c.floor, frames.RECTS)
        assert again.tobytes() == whole.tobytes()  # and two calls give the same bytes
    for j, rect in enumerate(frames.RECTS):  # each rect is reduced on its own
        assert render.tile_error(ctx, fb, fb_sq, c.n, c.floor, [rect]).tobytes() == whole[j : j + 1].tobytes(), rect


# ---------------------------------------------------------------- rmd_tile_error_dual
def device_dual(ctx, err, rects):
    height, width = err.shape
    with render.ErrorImage(ctx, width, height) as img:
        img.upload(err)
        return render.tile_error_dual(ctx, img, rects)


def far_from(a, b):
    return abs(a - b) > 1e-3 * max(abs(a), abs(b))


@pytest.mark.parametrize("name", [c.name for c in frames.err_cases() + frames.wide_err_cases()])
def test_dual_follows_the_header_sum_order(gpu_ctx, name):
    c = frames.err_case(name)
    got = device_dual(gpu_ctx, c.err, c.rects)
    assert_follows(got, ref.tile_error_dual(c.err, c.rects), "dual " + name)
    for j in c.designated or ():  # the test could tell: the plain sum is far from what the device gave
        values = ref.rect_values(c.err, c.rects[j])
        with np.errstate(all="ignore"):
            plain = float(np.sqrt(np.float64(max(np.sum(values), 0.0)) / values.size))
        assert far_from(float(got[j]), plain), (name, c.rects[j], got[j], plain)
    if name.startswith("nan") or name == "inf":
        tile = c.rects.index(frames.TILE)
        assert got[tile] == np.inf and got[c.rects.index((0, 0, frames.W, frames.H))] == np.inf and np.isfinite(got).sum() > 6
    if name == "zeros":
        assert ref.same_bits(got, np.zeros(len(c.rects)))


def test_dual_totals_with_an_exact_root_are_exact(gpu_ctx):
    got = device_dual(gpu_ctx, frames.exact_image(), [r for r, _ in frames.EXACT_RECTS])
    assert ref.same_bits(got, np.array([w for _, w in frames.EXACT_RECTS])), got


def test_dual_position_and_frame_width_change_no_bit(gpu_ctx):
    for name, j in (("chain", 1), ("chain", 2), ("pairs", 0), ("pairs", 1), ("pairs", 2), ("positive", frames.RECTS.index((40, 1, 27, 19))),
                    ("positive", frames.RECTS.index(frames.TILE))):
        c = frames.err_case(name)
        l, t, w, h = c.rects[j]
        here = device_dual(gpu_ctx, c.err, [c.rects[j]])
        other = np.full((frames.WIDE, 91), 123.0)  # another width, another corner
        other[101 : 101 + h, 7 : 7 + w] = c.err[t : t + h, l : l + w]
        there = device_dual(gpu_ctx, other, [(7, 101, w, h)])
        assert ref.same_bits(here, there), (name, c.rects[j], here, there)


def test_dual_list_shapes(gpu_ctx):
    c = frames.err_case("positive")
    with render.ErrorImage(gpu_ctx, frames.W, frames.H) as img:
        img.upload(c.err)
        whole = render.tile_error_dual(gpu_ctx, img, c.rects)
        assert render.tile_error_dual(gpu_ctx, img, c.rects).tobytes() == whole.tobytes()
        for j, rect in enumerate(c.rects):  # each rect is summed on its own
            assert render.tile_error_dual(gpu_ctx, img, [rect]).tobytes() == whole[j : j + 1].tobytes(), rect
        keep = [j for j, r in enumerate(c.rects) if r[2] * r[3]]
        assert len(keep) == len(c.rects) - 3 and (whole[frames.EMPTY] == 0.0).all()
        assert render.tile_error_dual(gpu_ctx, img, [c.rects[j] for j in keep]).tobytes() == whole[keep].tobytes()  # the rects without pixels shift nothing
        assert len(render.tile_error_dual(gpu_ctx, img, [])) == 0


# ---------------------------------------------------------------- the decision at equality
TILE_SIZE = 16


def first_check_at_or_below(errors, i, thr):
    return next((c for c in sorted(errors) if errors[c][i] <= thr), moments.ASPP)


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return moments.CLI


@pytest.fixture(scope="module")
def reference(gpu_ctx):
    """moments.uniform_reference on 16 x 16 tiles, and the tile and check whose error serves as the threshold: one that first falls to it at a later check
    than the first, so that `<=` is asked after `>` has been answered, and with other tiles on either side."""
    tiles, frames_at, errors = moments.uniform_reference(gpu_ctx, (TILE_SIZE, TILE_SIZE))
    checks = sorted(errors)
    found = []
    for i in range(len(tiles)):
        for k, c in enumerate(checks[1:], 1):
            e = float(errors[c][i])
            if e > 0.0 and all(errors[c2][i] > e for c2 in checks[:k]):
                found.append((e, i, c))
    assert found
    thr, i, c = sorted(found)[len(found) // 2]
    return tiles, frames_at, errors, thr, i, c


def expected_frame(tiles, frames_at, errors, thr):
    """The frame a `<=` loop delivers: every tile's sums at the first check at or below thr, divided by that count."""
    img = np.zeros((moments.AH, moments.AW, 3))
    counts = []
    for i, (l, t, w, h) in enumerate(tiles):
        c = first_check_at_or_below(errors, i, thr)
        counts.append(c)
        img[t : t + h, l : l + w] = frames_at[c][t : t + h, l : l + w] / float(c)
    return img, counts


def adaptive_settings(thr):
    return Settings(scenes.camera(moments.AW, moments.AH), sample_count=moments.ASPP, bounce_limit=5, seed=scenes.SEED, tile_size=(TILE_SIZE, TILE_SIZE),
                    samples_per_iteration=moments.ASPI, adaptive_threshold=thr)


def test_render_tiled_finishes_a_tile_whose_error_equals_the_threshold(reference):
    tiles, frames_at, errors, thr, i, c = reference
    below = float(np.nextafter(thr, 0.0))  # to this threshold the tile's error at check c is the next double above
    assert first_check_at_or_below(errors, i, thr) == c and first_check_at_or_below(errors, i, below) > c
    for threshold in (thr, below):
        h = render.render_tiled(scenes.reflective_spheres(), adaptive_settings(threshold))
        finished = {(m.tile.left, m.tile.top, m.tile.width, m.tile.height): m.tile for m in h._messages if m.kind == "TileFinished"}
        want_img, want_counts = expected_frame(tiles, frames_at, errors, threshold)
        assert [finished[r].sample_count for r in tiles] == want_counts
        mine = finished[tiles[i]]
        if threshold == thr:
            assert mine.sample_count == c and mine.error == thr
        else:
            assert mine.sample_count > c
            at_c = [m.tile for m in h._messages if m.kind == "TileProgressed" and m.tile.sample_count == c and (m.tile.left, m.tile.top) == tiles[i][:2]]
            assert len(at_c) == 1 and at_c[0].error == thr  # checked there, one double above the threshold, and sent on
        h.async_await()
        assert h.await_().tobytes() == want_img.tobytes()


def test_raymond_cli_decides_at_equality_as_render_tiled_does(reference, cli, tmp_path):
    tiles, frames_at, errors, thr, i, c = reference
    made = []
    for threshold in (thr, float(np.nextafter(thr, 0.0))):
        raw = tmp_path / ("%d.f64" % len(made))
        r = subprocess.run([cli, "render", "spheres", str(moments.AW), str(moments.AH), str(moments.ASPP), "5", str(tmp_path / "o.ppm"), "--raw", str(raw),
                            "--spi", str(moments.ASPI), "--tile-size", str(TILE_SIZE), "--adaptive", repr(threshold)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        img = np.fromfile(raw).reshape(moments.AH, moments.AW, 3)
        assert img.tobytes() == expected_frame(tiles, frames_at, errors, threshold)[0].tobytes()
        made.append(img)
    l, t, w, h = tiles[i]
    assert made[0][t : t + h, l : l + w].tobytes() == (frames_at[c][t : t + h, l : l + w] / float(c)).tobytes()
    assert made[0][t : t + h, l : l + w].tobytes() != made[1][t : t + h, l : l + w].tobytes()
