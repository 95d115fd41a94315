"""rmd_despike on the GPU: both outputs and the per-rect counts byte for byte against the numpy restatement (tests/despike_ref.py, which
tests/test_despike_host.py holds to hand-derived outcomes) on random frames — a smooth base, exact-tie plateaus, planted spikes, pairs and lines, negative,
NaN and inf sums, four rects at counts 2, 5, 16 and 16, a count-1 rect and an uncovered strip — at sizes on both sides of the kernel's 32 x 16 workgroup tile
(1 x 1, 3 x 2; 37 x 21 = one tile and a remainder of 5 each way; 131 x 70 = four tiles and remainders of 3 and 6), every radius, the ranks 0, 2 and the
largest, ratio 1 and 2, k 0 and 6, floor 0 and a floor above every spike; sentinels around both outputs; a repeated call; the hand-derived classes;
rmd_tile_error on the planted-firefly tile before and after; and settings.despike through await_() and the adaptive loop."""
import os
import subprocess

import numpy as np
import pytest

import despike_frames as frames
import despike_ref as ref
from raymond_amd import render, scenes
from raymond_amd.scene import Settings, generate_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")

SIZES = [(1, 1), (3, 2), (37, 21), (131, 70)]
SENTINEL = np.uint64(0x7FF8DEADBEEF0001).view(np.float64)  # a NaN no arithmetic makes


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Guarded:
    """A W x H framebuffer inside a larger allocation whose other doubles hold SENTINEL: a guard of one row (at least 3 doubles) on either side."""

    def __init__(self, ctx, width, height):
        self.ctx, self.width, self.height = ctx, width, height
        self.whole = render.Framebuffer(ctx, width, height + 2)
        self.whole.upload(np.full((height + 2, width, 3), SENTINEL))
        self.fb = render.Framebuffer(ctx, width, height, device_ptr=self.whole.ptr.value + width * 3 * 8)

    def read(self):
        """The frame; asserts that both guards are intact."""
        all_of_it = self.whole.download()
        assert (bits(all_of_it[0]) == bits(SENTINEL)).all() and (bits(all_of_it[-1]) == bits(SENTINEL)).all(), "a write outside the W*H*3 range"
        return all_of_it[1:-1].copy()

    def close(self):
        self.whole.close()


class Device:
    """One frame on the device, despiked into guarded outputs as often as wanted."""

    def __init__(self, ctx, S, Q, rects, counts):
        self.ctx, self.rects, self.counts = ctx, rects, counts
        H, W = S.shape[0], S.shape[1]
        self.S, self.Q = render.Framebuffer(ctx, W, H), render.Framebuffer(ctx, W, H)
        self.S.upload(S), self.Q.upload(Q)
        self.oS, self.oQ = Guarded(ctx, W, H), Guarded(ctx, W, H)

    def despike(self, **params):
        _, _, replaced = render.despike(self.ctx, self.S, self.Q, self.rects, self.counts, out=(self.oS.fb, self.oQ.fb), **params)
        return self.oS.read(), self.oQ.read(), replaced

    def close(self):
        for b in (self.S, self.Q, self.oS, self.oQ):
            b.close()


def same_as_ref(got, want, what):
    gS, gQ, g_replaced = got
    wS, wQ, w_replaced, spikes = want
    bad = np.argwhere((bits(gS) != bits(wS)).any(axis=2) | (bits(gQ) != bits(wQ)).any(axis=2))
    assert bad.size == 0, (what, "pixels (y, x) that differ", bad[:8].tolist(), "spikes of the restatement", spikes[:8])
    assert list(g_replaced) == list(w_replaced), (what, list(g_replaced), list(w_replaced))


@pytest.fixture(scope="module")
def random_frames():
    return {size: frames.random_frame(size[0], size[1], seed=7) for size in SIZES}


@pytest.mark.parametrize("rank_kind", ["rank0", "rank2", "rank_max"])
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_byte_for_byte_against_the_restatement(gpu_ctx, random_frames, size, radius, rank_kind):
    S, Q, rects, counts = random_frames[size]
    rank = {"rank0": 0, "rank2": 2, "rank_max": (2 * radius + 1) ** 2 - 2}[rank_kind]
    plan = ref.Plan(S, Q, rects, counts, radius, rank)
    dev = Device(gpu_ctx, S, Q, rects, counts)
    try:
        found = 0
        for ratio in (1.0, 2.0):
            for k in (0.0, 6.0):
                for floor in (0.0, 1e300):
                    params = dict(radius=radius, rank=rank, k=k, ratio=ratio, floor=floor)
                    want = plan.decide(k, ratio, floor)
                    got = dev.despike(**params)
                    same_as_ref(got, want, params)
                    if floor > 0.0:  # above every spike: nothing is replaced and the outputs are the input's bytes
                        assert want[3] == [] and ref.same_bits(got[0], S) and ref.same_bits(got[1], Q) and not got[2].any()
                    found += len(want[3])
        print("%dx%d radius %d rank %d: %d spikes over the eight settings" % (size[0], size[1], radius, rank, found))
        if size[0] * size[1] > 100 and rank < (2 * radius + 1) ** 2 - 2:
            assert found > 0  # (the planted spikes are found: the comparison is not one of untouched frames)
    finally:
        dev.close()


def test_two_calls_in_a_row_give_the_same_bytes_and_counts_are_optional(gpu_ctx, random_frames):
    S, Q, rects, counts = random_frames[(37, 21)]
    dev = Device(gpu_ctx, S, Q, rects, counts)
    try:
        first = dev.despike()
        second = dev.despike()
        assert ref.same_bits(first[0], second[0]) and ref.same_bits(first[1], second[1]) and list(first[2]) == list(second[2]) and first[2].sum() > 0
        # another setting in between leaves nothing behind in the context's scratch
        dev.despike(radius=3, rank=0, k=0.0, ratio=1.0)
        third = dev.despike()
        assert ref.same_bits(first[0], third[0]) and ref.same_bits(first[1], third[1]) and list(first[2]) == list(third[2])
        # without the counts (replaced_host NULL) the frames are the same
        render.despike(gpu_ctx, dev.S, dev.Q, rects, counts, out=(dev.oS.fb, dev.oQ.fb), want_replaced=False)
        assert ref.same_bits(dev.oS.read(), first[0]) and ref.same_bits(dev.oQ.read(), first[1])
        # and without rects nothing is valid: a copy
        oS, oQ, replaced = render.despike_arrays(gpu_ctx, S, Q, [], [])
        assert ref.same_bits(oS, S) and ref.same_bits(oQ, Q) and len(replaced) == 0
    finally:
        dev.close()


def test_the_hand_derived_classes_through_the_device(gpu_ctx):
    """The frames of tests/test_despike_host.py: the device gives the restatement's bytes, and the counts derived there by hand."""
    W = H = 12
    one = [(0, 0, W, H)]

    def run(S, Q, rects, counts, expect_replaced, **params):
        want = ref.despike(S, Q, rects, counts, **params)
        dev = Device(gpu_ctx, S, Q, rects, counts)
        try:
            got = dev.despike(**params)
        finally:
            dev.close()
        same_as_ref(got, want, params)
        assert list(got[2]) == expect_replaced, (params, list(got[2]))
        return got

    S, Q, rects, counts = frames.flat(W, H)  # constant
    run(S, Q, rects, counts, [0], k=0.0, ratio=1.0, floor=0.0)
    rS, rQ = frames.sums_of(1.0 + np.arange(W)[None, :] / 8.0 + np.zeros((H, 1)), 16)  # the ramp: its two right-hand corners at ratio 1, nothing at 2
    run(rS, rQ, rects, counts, [2], k=0.0, ratio=1.0, floor=0.0)
    run(rS, rQ, rects, counts, [0])
    S, Q, _, _ = frames.flat(W, H)  # an isolated spike, in the second rect
    frames.plant(S, Q, 7, 5, 50.0)
    oS, oQ, _ = run(S, Q, [(0, 0, 6, H), (6, 0, 6, H)], [16, 16], [0, 1])
    assert np.array_equal(bits(oS)[5, 7], bits(S)[3, 7]) and np.array_equal(bits(oQ)[5, 7], bits(Q)[3, 7])
    S, Q, _, _ = frames.flat(W, H)  # a pair
    frames.plant(S, Q, 5, 5, 50.0), frames.plant(S, Q, 6, 5, 50.0)
    run(S, Q, one, [16], [0], rank=0)
    oS, oQ, _ = run(S, Q, one, [16], [2], rank=1)
    assert np.array_equal(bits(oQ)[5, 5], bits(Q)[3, 3]) and np.array_equal(bits(oQ)[5, 6], bits(Q)[3, 4])  # each from the INPUT
    S, Q, _, _ = frames.flat(W, H)  # a one-pixel line
    for y in range(H):
        frames.plant(S, Q, 6, y, 50.0)
    run(S, Q, one, [16], [2], radius=2, rank=2)  # (its two ends)
    oS, _, _ = run(S, Q, one, [16], [H], radius=1, rank=2)
    assert (oS[:, 6] == 16.0).all()
    S, Q, _, _ = frames.flat(W, H)  # the corner
    frames.plant(S, Q, 0, 0, 50.0)
    run(S, Q, one, [16], [1], radius=1, rank=2)
    run(S, Q, one, [16], [0], radius=1, rank=3)
    S, Q, _, _ = frames.flat(W, H)  # pixels that are not valid: never donors, copied with their payloads
    frames.plant(S, Q, 5, 5, 50.0)
    for rects, counts, expect in (([(0, 0, W, 4), (0, 4, W, H - 4)], [1, 16], [0, 1]), ([(0, 4, W, H - 4)], [16], [1])):
        oS, oQ, _ = run(S, Q, rects, counts, expect)
        assert np.array_equal(bits(oQ)[5, 5], bits(Q)[4, 5])
    S[3, 3, 1] = np.uint64(0x7FF8000000000123).view(np.float64)
    Q[3, 4, 2] = np.inf
    oS, oQ, _ = run(S, Q, one, [16], [1])
    assert np.array_equal(bits(oQ)[5, 5], bits(Q)[3, 7]) and bits(oS)[3, 3, 1] == np.uint64(0x7FF8000000000123)
    n = np.full((H, W), 16.0)  # a donor at another count: the scaled copy, to the bit
    n[:4] = 5.0
    S, Q = frames.sums_of(np.ones((H, W)), n, frames.S2 * (1.0 + 1e-3 * np.arange(W * H, dtype=np.float64).reshape(H, W)))
    frames.plant(S, Q, 5, 5, 50.0)
    oS, oQ, _ = run(S, Q, [(0, 0, W, 4), (0, 4, W, H - 4)], [5, 16], [0, 1])
    for c in range(3):
        assert oS[5, 5, c] == 16.0 and bits(oQ)[5, 5, c] == bits(np.array((Q[3, 5, c] / np.float64(5.0)) * np.float64(16.0)))
    S, Q, _, _ = frames.flat(W, H, value=-1.0)  # a negative donor luminance
    frames.plant(S, Q, 5, 5, -1.5)
    oS, oQ, _ = run(S, Q, one, [16], [W * H])
    assert np.array_equal(bits(oQ)[5, 5], bits(Q)[3, 5])
    run(S, Q, one, [16], [0], ratio=1.0)


def test_tile_error_on_the_planted_firefly_tile_before_and_after(gpu_ctx):
    """The tile the stage exists for, through render.tile_error: above the threshold on S, Q, at or below it on S', Q' — as the restatement says."""
    W = H = 12
    S, Q, rects, counts = frames.flat(W, H)
    S[6, 4] = 15.0 + 800.0
    Q[6, 4] = 15.0 * (1.0 + frames.S2) + 800.0 * 800.0
    threshold, floor = 0.05, 1e-3
    fbs = [render.Framebuffer(gpu_ctx, W, H) for _ in range(2)]
    clean = []
    try:
        fbs[0].upload(S), fbs[1].upload(Q)
        before = render.tile_error(gpu_ctx, fbs[0], fbs[1], 16, floor, rects)[0]
        cS, cQ, replaced = render.despike(gpu_ctx, fbs[0], fbs[1], rects, counts)
        clean = [cS, cQ]
        after = render.tile_error(gpu_ctx, cS, cQ, 16, floor, rects)[0]
        print("rmd_tile_error before %.6g, after %.6g" % (before, after))
        assert list(replaced) == [1] and before > threshold >= after
        want = ref.despike(S, Q, rects, counts)
        assert abs(before - ref.tile_error(S, Q, 16, floor, rects)[0]) <= 1e-12 * before and abs(after - ref.tile_error(want[0], want[1], 16, floor, rects)[0]) <= 1e-12 * after
    finally:
        for b in fbs + clean:
            b.close()


# ---------------------------------------------------------------- settings.despike through the render loops
def small_settings(**kw):
    return Settings(scenes.camera(64, 48), 8, bounce_limit=3, seed=scenes.SEED, **kw)


def finished_frame(handle):
    """The finished tiles of a handle that has not been awaited yet, assembled: (S, Q, rects, counts); the messages stay."""
    cam = handle.settings.camera_settings
    shape = (cam.backbuffer_height, cam.backbuffer_width, 3)
    S, Q, rects, counts = np.zeros(shape), np.zeros(shape), [], []
    for m in handle._messages:
        if m.kind != "TileFinished":
            continue
        t = m.tile
        assert t.data_sq is not None  # with despike on the passes render with moments and the finished tiles carry them
        S[t.top : t.top + t.height, t.left : t.left + t.width] = t.data
        Q[t.top : t.top + t.height, t.left : t.left + t.width] = t.data_sq
        rects.append((t.left, t.top, t.width, t.height))
        counts.append(t.sample_count)
    return S, Q, rects, counts


@pytest.mark.parametrize("path", ["plain", "denoise_atrous"])
def test_await_is_despike_followed_by_the_existing_path(gpu_ctx, path):
    scene = scenes.reflective_spheres()
    extra = dict(denoise=True, denoise_atrous=True, denoise_atrous_levels=3) if path == "denoise_atrous" else {}
    # k 0, ratio 1: every local maximum above its third-brightest other is replaced — the stage has work to do on an 8 spp frame
    st = small_settings(despike=True, despike_k=0.0, despike_ratio=1.0, **extra)
    handle = render.render_tiled(scene, st)
    S, Q, rects, counts = finished_frame(handle)
    got = handle.await_()
    dS, dQ, replaced = render.despike_arrays(gpu_ctx, S, Q, rects, counts, **st.despike_keywords())
    assert replaced.sum() > 0 and not ref.same_bits(dS, S)
    if path == "plain":
        want = np.zeros_like(S)
        for (l, t, w, h), n in zip(rects, counts):
            want[t : t + h, l : l + w] = dS[t : t + h, l : l + w] / float(n)
    else:
        want = render.denoise_atrous_arrays(gpu_ctx, dS, dQ, None, None, rects, counts, levels=3, k=st.denoise_atrous_k, alpha=st.denoise_alpha)
    assert ref.same_bits(got, want)
    # the tiles carried the raw sums: a render without the setting delivers the same data
    off = render.render_tiled(scene, small_settings(**extra))
    raw = {(m.tile.left, m.tile.top): m.tile.data for m in off._messages if m.kind == "TileFinished"}
    for (l, t, w, h) in rects:
        assert ref.same_bits(raw[(l, t)], S[t : t + h, l : l + w])
    # a floor above every spike: the frame is the bytes of despike off
    high = render.render_tiled(scene, small_settings(despike=True, despike_k=0.0, despike_ratio=1.0, despike_floor=1e300, **extra)).await_()
    assert ref.same_bits(high, off.await_()) and not ref.same_bits(high, got)


def test_the_adaptive_run_with_despike_ends_and_its_tiles_hold_raw_sums(gpu_ctx):
    scene = scenes.reflective_spheres()
    # (4 x 4 tiles: some lie wholly on the unlit wall and finish at the first check, so the check's rect list holds finished tiles at their own counts
    # beside the live ones)
    st = Settings(scenes.camera(64, 48), 16, tile_size=(4, 4), bounce_limit=3, seed=scenes.SEED, samples_per_iteration=4, adaptive_threshold=0.5, despike=True)
    handle = render.render_tiled(scene, st)
    done = [m.tile for m in handle._messages if m.kind == "TileFinished"]
    tiles = generate_tiles(64, 48, st.tile_size)
    assert len(tiles) == 192 and sorted((t.left, t.top, t.width, t.height) for t in done) == sorted(tiles)  # every tile, once
    assert all(t.sample_count % 4 == 0 and 4 <= t.sample_count <= 16 and t.data_sq is not None for t in done)
    assert any(t.sample_count < 16 for t in done) and any(t.sample_count == 16 for t in done)  # (the unlit tiles stop at once, the lit ones never)
    print("finished tiles per sample count:", {c: sum(1 for t in done if t.sample_count == c) for c in (4, 8, 12, 16)})
    # a finished tile's bytes are those of a plain render of that tile in the same passes: nothing the check wrote went into the sums
    cam = st.camera_settings
    ds = render.DeviceScene(gpu_ctx, scene)
    fb, fb_sq = render.Framebuffer(gpu_ctx, 64, 48), render.Framebuffer(gpu_ctx, 64, 48)
    try:
        for t in (min(done, key=lambda t: t.sample_count), max(done, key=lambda t: t.sample_count)):
            rect = (t.left, t.top, t.width, t.height)
            fb.zero(), fb_sq.zero()
            for begin in range(0, t.sample_count, 4):
                render.render_tiles(gpu_ctx, ds, cam, st, [rect], fb, begin, 4, framebuffer_sq=fb_sq)
            assert ref.same_bits(fb.download_tiles([rect])[0], t.data) and ref.same_bits(fb_sq.download_tiles([rect])[0], t.data_sq)
    finally:
        fb.close(), fb_sq.close(), ds.close()
    assert handle.await_().shape == (48, 64, 3)


@pytest.mark.parametrize("extra", [[], ["--denoise", "1", "--denoise-atrous", "1", "--denoise-atrous-levels", "3"], ["--denoise", "1", "--denoise-radius", "3", "--denoise-patch", "1"],
                                   ["--adaptive", "0.99"]], ids=["plain", "denoise_atrous", "denoise", "adaptive"])
def test_cli_equals_the_python_path(gpu_ctx, tmp_path, extra):
    """The C++ mirror through raymond_cli --despike 1: await()'s plain divide and filters, and the adaptive check, give the Python path's bytes."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    W, H, spp, bounces = 64, 48, 12, 3
    ppm, raw = tmp_path / "o.ppm", tmp_path / "o.f64"
    r = subprocess.run([CLI, "render", "spheres", str(W), str(H), str(spp), str(bounces), str(ppm), "--raw", str(raw), "--spi", "4", "--despike", "1", "--despike-k", "0",
                        "--despike-ratio", "1", "--despike-radius", "1", "--despike-rank", "1", *extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img_cpp = np.fromfile(raw).reshape(H, W, 3)
    opts = dict(zip(extra[0::2], extra[1::2]))
    st = Settings(scenes.camera(W, H), sample_count=spp, tile_size=(32, 32), bounce_limit=bounces, seed=scenes.SEED, samples_per_iteration=4, despike=True, despike_k=0.0,
                  despike_ratio=1.0, despike_radius=1, despike_rank=1, denoise="--denoise" in opts, denoise_atrous="--denoise-atrous" in opts,
                  denoise_atrous_levels=int(opts.get("--denoise-atrous-levels", 5)), denoise_radius=int(opts.get("--denoise-radius", 10)),
                  denoise_patch=int(opts.get("--denoise-patch", 3)), adaptive_threshold=float(opts.get("--adaptive", 0.0)))
    handle = render.render_tiled(scenes.reflective_spheres(), st, devices=(0,))
    handle.async_await()
    img_py = handle.await_()
    assert img_cpp.tobytes() == img_py.tobytes()
    off = render.render_tiled(scenes.reflective_spheres(), Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=bounces, seed=scenes.SEED, samples_per_iteration=4))
    off.async_await()
    assert off.await_().tobytes() != img_py.tobytes()  # (the stage had work to do)
