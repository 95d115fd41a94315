"""rmd_despike_dual on the GPU: all twelve output planes and the per-rect counts byte for byte against the numpy restatement (tests/despike_dual_ref.py, which
tests/test_despike_dual_host.py holds to hand-derived outcomes and tells from four wrong readings) on the random frames of tests/despike_dual_frames.py —
rects at (n_A, n_B) = (8, 8), (8, 16), (1, 1), (0, 8), an uncovered strip, fireflies in one half, ties, negatives, NaN and infinities in one half only,
halves whose sum overflows — at sizes on both sides of the kernel's 32 x 16 workgroup tile, every radius, the ranks 0, 2 and the largest; outputs pre-filled
with a sentinel NaN inside guards; replaced_host NULL and a repeated call; the hand-derived classes; the two statements the definition makes true against
rmd_despike on the device; the purpose — a planted firefly's tile through rmd_denoise_dual and rmd_tile_error_dual, before and after —; and
settings.despike_dual through the Python dual loop, await_() and raymond_cli."""
import os
import subprocess

import numpy as np
import pytest

import despike_dual_frames as frames
import despike_dual_ref as ref
from raymond_amd import render, scenes
from raymond_amd.scene import Settings, generate_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
SENTINEL = np.uint64(0x7FF8DEADBEEF0001).view(np.float64)  # a NaN no arithmetic makes


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Guarded:
    """A W x H framebuffer inside a larger allocation whose every double holds SENTINEL: the frame itself, and a guard of one row (at least 3 doubles) on
    either side."""

    def __init__(self, ctx, width, height):
        self.whole = render.Framebuffer(ctx, width, height + 2)
        self.fb = render.Framebuffer(ctx, width, height, device_ptr=self.whole.ptr.value + width * 3 * 8)
        self.fill()

    def fill(self):
        self.whole.upload(np.full((self.fb.height + 2, self.fb.width, 3), SENTINEL))

    def read(self):
        """The frame; asserts that both guards are intact."""
        all_of_it = self.whole.download()
        assert (bits(all_of_it[0]) == bits(SENTINEL)).all() and (bits(all_of_it[-1]) == bits(SENTINEL)).all(), "a write outside the W*H*3 range"
        return all_of_it[1:-1].copy()

    def close(self):
        self.whole.close()


class Device:
    """One dual frame on the device, despiked into guarded, sentinel-filled outputs as often as wanted."""

    def __init__(self, ctx, SA, QA, SB, QB, rects, counts_a, counts_b):
        self.ctx, self.rects, self.counts_a, self.counts_b = ctx, rects, counts_a, counts_b
        H, W = SA.shape[0], SA.shape[1]
        self.inputs = [render.Framebuffer(ctx, W, H) for _ in range(4)]
        for fb, a in zip(self.inputs, (SA, QA, SB, QB)):
            fb.upload(a)
        self.outs = [Guarded(ctx, W, H) for _ in range(4)]

    def despike(self, **params):
        for g in self.outs:
            g.fill()
        out = ((self.outs[0].fb, self.outs[1].fb), (self.outs[2].fb, self.outs[3].fb))
        _, _, replaced = render.despike_dual(self.ctx, self.inputs[0:2], self.inputs[2:4], self.rects, self.counts_a, self.counts_b, out=out, **params)
        return tuple(g.read() for g in self.outs) + (replaced,)

    def close(self):
        for b in self.inputs + self.outs:
            b.close()


def same_as_ref(got, want, what):
    bad = np.zeros(got[0].shape[:2], dtype=bool)
    for g, w in zip(got[:4], want[:4]):
        bad |= (bits(g) != bits(w)).any(axis=2)
    assert not bad.any(), (what, "pixels (y, x) that differ", np.argwhere(bad)[:8].tolist(), "spikes of the restatement", want[5][:8])
    if got[4] is not None:
        assert [int(v) for v in got[4]] == [int(v) for v in want[4]], (what, list(got[4]), list(want[4]))


@pytest.mark.parametrize("radius", frames.RADII)
@pytest.mark.parametrize("size", frames.SIZES, ids=["%dx%d" % s for s in frames.SIZES])
def test_byte_for_byte_against_the_restatement(gpu_ctx, size, radius):
    SA, QA, SB, QB, rects, ca, cb = frames.frame(size)
    dev = Device(gpu_ctx, SA, QA, SB, QB, rects, ca, cb)
    try:
        found = 0
        for rank in frames.ranks(radius):
            want = frames.reference(size, radius, rank)
            same_as_ref(dev.despike(radius=radius, rank=rank), want, (size, radius, rank))
            found += len(want[5])
        # a floor above every spike: nothing is replaced and every output is its input's bytes — every pixel is written, the sentinels are gone
        got = dev.despike(radius=radius, rank=0, floor=1e300)
        assert all(ref.same_bits(g, a) for g, a in zip(got[:4], (SA, QA, SB, QB))) and not got[4].any()
        print("%dx%d radius %d: %d spikes over the three ranks" % (size[0], size[1], radius, found))
        assert found > 0 or size[0] * size[1] < 100  # (the planted spikes are found: the comparison is not one of untouched frames)
    finally:
        dev.close()


def test_counts_are_optional_and_a_repeated_call_gives_the_same_bytes(gpu_ctx):
    size = (37, 21)
    SA, QA, SB, QB, rects, ca, cb = frames.frame(size)
    want = frames.reference(size, 2, 2)
    dev = Device(gpu_ctx, SA, QA, SB, QB, rects, ca, cb)
    try:
        first = dev.despike()
        same_as_ref(first, want, "first")
        assert first[4].sum() > 0
        dev.despike(radius=3, rank=0, k=0.0, ratio=1.0)  # another setting in between leaves nothing behind in the context's scratch
        second = dev.despike()
        same_as_ref(second, want, "repeated")
        without = dev.despike(want_replaced=False)  # replaced_host NULL: the same bytes
        assert without[4] is None
        same_as_ref(without, want, "replaced_host NULL")
        got = render.despike_dual_arrays(gpu_ctx, SA, QA, SB, QB, [], [], [])  # without rects nothing is valid: a copy
        assert all(ref.same_bits(g, a) for g, a in zip(got[:4], (SA, QA, SB, QB))) and len(got[4]) == 0
    finally:
        dev.close()


@pytest.mark.parametrize("name", sorted(frames.HAND))
def test_the_hand_derived_classes_through_the_device(gpu_ctx, name):
    planes, expected = frames.HAND[name]
    want = ref.despike_dual(*planes, frames.HAND_RECTS, frames.HAND_A, frames.HAND_B)
    assert sorted(want[5]) == sorted(expected)
    dev = Device(gpu_ctx, *planes, frames.HAND_RECTS, frames.HAND_A, frames.HAND_B)
    try:
        got = dev.despike()
    finally:
        dev.close()
    same_as_ref(got, want, name)
    frames.check_hand(name, planes, got)


# ---------------------------------------------------------------- the two statements, against rmd_despike on the device itself
def changed_pixels(outputs, inputs):
    changed = np.zeros(inputs[0].shape[:2], dtype=bool)
    for o, i in zip(outputs, inputs):
        changed |= (bits(o) != bits(i)).any(axis=2)
    return changed


@pytest.mark.parametrize("radius,rank", [(1, 0), (2, 2), (3, 47)])
def test_statement_a_the_spikes_are_rmd_despikes_on_all_the_samples(gpu_ctx, radius, rank):
    ca, cb = [8, 8, 1, 8, 3], [8, 16, 1, 8, 8]  # every rect with both counts >= 1
    SA, QA, SB, QB, rects, _, _ = frames.random_frame(37, 21, seed=11, counts=(ca, cb))
    S, Q = ref.merge(SA, QA, SB, QB)
    dual = render.despike_dual_arrays(gpu_ctx, SA, QA, SB, QB, rects, ca, cb, radius=radius, rank=rank)
    oS, oQ, replaced = render.despike_arrays(gpu_ctx, S, Q, rects, [a + b for a, b in zip(ca, cb)], radius=radius, rank=rank)
    assert [int(v) for v in dual[4]] == [int(v) for v in replaced] and replaced.sum() > 0
    # (every pixel of these frames has bits of its own in Q, so a replaced pixel is a changed pixel)
    assert np.array_equal(changed_pixels(dual[:4], (SA, QA, SB, QB)), changed_pixels((oS, oQ), (S, Q)))


@pytest.mark.parametrize("radius,rank", [(1, 0), (2, 2), (3, 47)])
def test_statement_b_the_halves_add_to_rmd_despikes_outputs(gpu_ctx, radius, rank):
    ca, cb = [8] * 5, [16] * 5  # ... and every spike's counts agree with its donor's, half by half
    SA, QA, SB, QB, rects, _, _ = frames.random_frame(37, 21, seed=12, counts=(ca, cb))
    S, Q = ref.merge(SA, QA, SB, QB)
    dual = render.despike_dual_arrays(gpu_ctx, SA, QA, SB, QB, rects, ca, cb, radius=radius, rank=rank)
    oS, oQ, replaced = render.despike_arrays(gpu_ctx, S, Q, rects, [24] * 5, radius=radius, rank=rank)
    assert [int(v) for v in dual[4]] == [int(v) for v in replaced] and replaced.sum() > 0
    mS, mQ = ref.merge(*dual[:4])
    assert ref.same_bits(mS, oS) and ref.same_bits(mQ, oQ)


# ---------------------------------------------------------------- the purpose
def test_the_fireflys_tile_before_and_after(gpu_ctx):
    """A flat frame in 16 x 16 tiles at (8, 8), one firefly planted in half A in the middle of tile 4 of 9: after rmd_denoise_dual the tile's
    rmd_tile_error_dual stands far above its neighbours'; after rmd_despike_dual it equals the unplanted frame's."""
    W = H = 48
    tiles = generate_tiles(W, H, (16, 16))
    counts = [8] * len(tiles)
    planted_tile = tiles.index((16, 16, 16, 16))
    params = dict(radius=3, patch_radius=1)

    def tile_errors(planes):
        _, err = render.denoise_dual_arrays(gpu_ctx, *planes, tiles, counts, counts, **params)
        img = render.ErrorImage(gpu_ctx, W, H)
        try:
            img.upload(err)
            return render.tile_error_dual(gpu_ctx, img, tiles)
        finally:
            img.close()

    flat = frames.flat_dual(W, H, [(0, 0, W, H)], [8], [8])
    planted = [a.copy() for a in flat]
    frames.plant_half(planted[0], planted[1], 24, 24, frames.FIREFLY, 8)
    unplanted, before = tile_errors(flat), tile_errors(planted)
    clean = render.despike_dual_arrays(gpu_ctx, *planted, tiles, counts, counts)
    assert [int(v) for v in clean[4]] == [1 if j == planted_tile else 0 for j in range(len(tiles))]
    after = tile_errors(clean[:4])
    print("rmd_tile_error_dual unplanted", unplanted.tolist(), "\nbefore", before.tolist(), "\nafter", after.tolist())
    others = [j for j in range(len(tiles)) if j != planted_tile]
    assert before[planted_tile] > 0.1 and all(before[j] < 1e-3 * before[planted_tile] for j in others)
    assert after[planted_tile] == unplanted[planted_tile] and all(after[j] == unplanted[j] for j in others)


# ---------------------------------------------------------------- settings.despike_dual through the dual loop
LW, LH, LSPP, LSPI, LMIN, LBOUNCES = 64, 48, 48, 8, 16, 3
FILTERS = {"default": dict(), "atrous_region": dict(denoise_dual_atrous=True, denoise_dual_atrous_region=True, denoise_atrous_levels=3)}


def loop_settings(threshold, **kw):
    return Settings(scenes.camera(LW, LH), LSPP, tile_size=(16, 16), bounce_limit=LBOUNCES, seed=scenes.SEED, samples_per_iteration=LSPI, denoise=True, denoise_dual=True,
                    denoise_radius=3, denoise_patch=1, adaptive_denoised_threshold=threshold, adaptive_min_samples=LMIN, **kw)


def finished_tiles(handle):
    return [m.tile for m in handle._messages if m.kind == "TileFinished"]


@pytest.mark.parametrize("which", sorted(FILTERS))
def test_the_python_loop_on_firefly_spheres(gpu_ctx, monkeypatch, which):
    scene = scenes.firefly_spheres()
    st = loop_settings(0.02, despike_dual=True, **FILTERS[which])
    all_tiles = generate_tiles(LW, LH, st.tile_size)
    despikes, filters = [], []
    real_despike, real_nlm, real_atrous = render.despike_dual, render.denoise_dual, render.denoise_atrous_dual

    def spy_despike(ctx, half_a, half_b, rects, counts_a, counts_b, **kw):
        despikes.append(dict(inputs=[b.ptr.value for b in tuple(half_a) + tuple(half_b)], rects=list(rects), a=list(counts_a), b=list(counts_b),
                             outs=[b.ptr.value for pair in kw["out"] for b in pair], want_replaced=kw.get("want_replaced")))
        return real_despike(ctx, half_a, half_b, rects, counts_a, counts_b, **kw)

    def spy_filter(real):
        def spy(ctx, half_a, half_b, rects, counts_a, counts_b, *args, **kw):
            filters.append(dict(halves=[b.ptr.value for b in tuple(half_a) + tuple(half_b)], rects=list(rects), a=list(counts_a), b=list(counts_b), region=kw.get("region"),
                                after=len(despikes)))
            return real(ctx, half_a, half_b, rects, counts_a, counts_b, *args, **kw)
        return spy

    monkeypatch.setattr(render, "despike_dual", spy_despike)
    monkeypatch.setattr(render, "denoise_dual", spy_filter(real_nlm))
    monkeypatch.setattr(render, "denoise_atrous_dual", spy_filter(real_atrous))
    handle = render.render_tiled(scene, st)
    monkeypatch.undo()
    done = finished_tiles(handle)
    assert sorted(t.rect for t in done) == sorted(all_tiles)
    print(which, "finished tiles per count:", {c: sum(1 for t in done if t.sample_count == c) for c in sorted({t.sample_count for t in done})})

    # once per checked pass — after 16 and 32 samples, while tiles are live —, over all tiles at their counts, into four buffers that are not the loop's own
    assert 1 <= len(despikes) <= 2 and len(filters) == len(despikes)
    for k, (d, f) in enumerate(zip(despikes, filters)):
        assert sorted(d["rects"]) == sorted(all_tiles) and d["want_replaced"] is False
        assert len(set(d["inputs"] + d["outs"])) == 8 and d["outs"] == despikes[0]["outs"] and d["inputs"] == despikes[0]["inputs"]
        live_a, live_b = (8, 8) if k == 0 else (16, 16)
        finished_before = {t.rect: (t.count_a, t.count_b) for t in done if t.sample_count < live_a + live_b}
        for rect, a, b in zip(d["rects"], d["a"], d["b"]):
            assert (a, b) == finished_before.get(rect, (live_a, live_b)), rect
        # the filter receives the spare buffers, right after that pass's despike call, at the same rects and counts, over the live tiles
        assert f["halves"] == d["outs"] and f["after"] == k + 1 and (f["rects"], f["a"], f["b"]) == (d["rects"], d["a"], d["b"])
        assert sorted(f["region"]) == sorted(r for r in all_tiles if r not in finished_before)

    # a finished tile carries RAW sums: its bytes are a replay of its passes, even ones into half A, odd ones into half B
    cam = st.camera_settings
    ds = render.DeviceScene(gpu_ctx, scene)
    fbs = [render.Framebuffer(gpu_ctx, LW, LH) for _ in range(4)]
    try:
        for t in (min(done, key=lambda t: t.sample_count), max(done, key=lambda t: t.sample_count)):
            for fb in fbs:
                fb.zero()
            for j, begin in enumerate(range(0, t.sample_count, LSPI)):
                half = j & 1
                render.render_tiles(gpu_ctx, ds, cam, st, [t.rect], fbs[2 * half], begin, LSPI, framebuffer_sq=fbs[2 * half + 1])
            for fb, data in zip(fbs, (t.data_a, t.data_sq_a, t.data_b, t.data_sq_b)):
                assert ref.same_bits(fb.download_tiles([t.rect])[0], data), t.rect
    finally:
        for b in fbs:
            b.close()
        ds.close()

    # await_() is despike_dual_arrays followed by the chosen filter's _arrays call
    halves = [np.zeros((LH, LW, 3)) for _ in range(4)]
    for t in done:
        for dst, src in zip(halves, (t.data_a, t.data_sq_a, t.data_b, t.data_sq_b)):
            t.put(dst, src)
    rects, ca, cb = [t.rect for t in done], [t.count_a for t in done], [t.count_b for t in done]
    handle.async_await()  # (the progress snapshots in front of the finished tiles)
    got = handle.await_()
    clean = render.despike_dual_arrays(gpu_ctx, *halves, rects, ca, cb, **st.despike_keywords())
    if which == "default":
        want, _ = render.denoise_dual_arrays(gpu_ctx, *clean[:4], rects, ca, cb, **st.nlm_keywords())
    else:
        want, _ = render.denoise_atrous_dual_arrays(gpu_ctx, *clean[:4], rects, ca, cb, **st.atrous_keywords())
    assert ref.same_bits(got, want)


def test_the_setting_off_makes_no_call_and_no_buffer(gpu_ctx, monkeypatch):
    calls = []
    monkeypatch.setattr(render, "despike_dual", lambda *a, **kw: calls.append(1))
    loops = []
    real_init = render._DualLoop.__init__

    def init(self, *a, **kw):
        real_init(self, *a, **kw)
        loops.append(self)

    monkeypatch.setattr(render._DualLoop, "__init__", init)
    render.render_tiled(scenes.reflective_spheres(), loop_settings(0.02))
    assert calls == [] and len(loops) == 1 and loops[0].spare is None


def test_cli_equals_the_python_loop(gpu_ctx, tmp_path):
    """raymond_cli render --despike-dual 1 on the bundled spheres scene (k 0, ratio 1: the stage has work to do on it): the Python loop's tiles, counts,
    deciding errors and --raw bytes."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    threshold = 0.02
    ppm, raw, dump = tmp_path / "o.ppm", tmp_path / "o.f64", tmp_path / "tiles.txt"
    r = subprocess.run([CLI, "render", "spheres", str(LW), str(LH), str(LSPP), str(LBOUNCES), str(ppm), "--raw", str(raw), "--spi", str(LSPI), "--tile-size", "16",
                        "--denoise", "1", "--denoise-dual", "1", "--denoise-radius", "3", "--denoise-patch", "1", "--adaptive-denoised", repr(threshold), "--adaptive-min",
                        str(LMIN), "--despike-dual", "1", "--despike-k", "0", "--despike-ratio", "1", "--dump-tiles", str(dump)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = {}
    for line in dump.read_text().strip().split("\n"):
        l, t, w, h, n, e = line.split()
        got[(int(l), int(t), int(w), int(h))] = (int(n), float(e))
    scene = scenes.reflective_spheres()
    handle = render.render_tiled(scene, loop_settings(threshold, despike_dual=True, despike_k=0.0, despike_ratio=1.0))
    done = {t.rect: t for t in finished_tiles(handle)}
    assert sorted(got) == sorted(done)
    for rect, tile in done.items():
        assert got[rect][0] == tile.sample_count, rect
        if tile.sample_count < LSPP:
            assert got[rect][1] == tile.error, rect  # the error that decided, the same bits
    handle.async_await()
    img = handle.await_()
    assert np.fromfile(raw).reshape(LH, LW, 3).tobytes() == img.tobytes()
    off = render.render_tiled(scene, loop_settings(threshold))
    off.async_await()
    assert off.await_().tobytes() != img.tobytes()  # (the stage had work to do)
