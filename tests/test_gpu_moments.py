"""Per-pixel second moments (rmd_render_tiles_moments), the per-tile error (rmd_tile_error) and adaptive render_tiled, on the GPU.

  * accum_sq is the ordered sum of the squared samples in every launch form, and accum is rmd_render_tiles' frame, bit for bit;
  * two calls over [0, k) and [k, n) give the bits of one call over [0, n); accum_sq = NULL is rmd_render_tiles;
  * rmd_tile_error equals its numpy restatement, special values included;
  * an adaptive render finishes converged tiles early with the sums of a uniform render at their count, and threshold 0 is today's render;
  * the C++ host mirror's adaptive render equals the Python one, bit for bit, with one and two workers.
"""
import os
import subprocess

import numpy as np
import pytest

from raymond_amd import abi, probe, render, scenes
from raymond_amd.scene import Settings, generate_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
W, H = 40, 24  # ragged wave tiles and host tiles
INFO_FIELDS = ("passes", "split_k", "persistent", "end_black_paths", "has_grid", "waves_per_workgroup", "buffered", "chained", "queued")


def info_tuple(ctx):
    i = ctx.last_launch_info()
    return tuple(getattr(i, f) for f in INFO_FIELDS)


def ordered_sums(ctx, ds, st, spp):
    """numpy's sum and sum of squares of every pixel's samples 0 .. spp-1, added in sample order, from the list-mode probe."""
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1), spp, axis=0)
    smp = np.tile(np.arange(spp, dtype=np.uint32), W * H)
    L = probe.trace_samples(ctx, ds, st.camera_settings, st, xy, smp).reshape(H * W, spp, 3)
    S, Q = np.zeros((H * W, 3)), np.zeros((H * W, 3))
    for s in range(spp):
        S = S + L[:, s]
        Q = Q + L[:, s] * L[:, s]
    return S.reshape(H, W, 3), Q.reshape(H, W, 3)


def run_form(ctx, ds, st, tiles, tunables, fb, fb_sq, with_sq=True, begin=0, count=None):
    for k, v in tunables.items():
        ctx.set_tunable(k, v)
    try:
        render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fb, begin, count, framebuffer_sq=fb_sq if with_sq else None)
        return info_tuple(ctx)
    finally:
        for k in tunables:
            ctx.set_tunable(k, 0)


T = abi
SPHERE_FORMS = [
    (12, {}),  # direct mode, one wave per item (a short launch of a scene without grids)
    (12, {T.RMD_TUNE_LAUNCH_FORM: 2}),  # direct mode, persistent
    (12, {T.RMD_TUNE_SAMPLE_SPLIT: 2}),  # role-sorted split launch, ordered sum in the kernel
    (12, {T.RMD_TUNE_SAMPLE_SPLIT: 4, T.RMD_TUNE_LAUNCH_FORM: 2}),
    (130, {}),  # >= kSortedMinSamples: buffered
    (130, {T.RMD_TUNE_LAUNCH_FORM: 1}),
    (130, {T.RMD_TUNE_LAUNCH_FORM: 2, T.RMD_TUNE_SAMPLE_SPLIT: 2}),
    (130, {T.RMD_TUNE_SCRATCH_CAP_MB: 1}),  # several scratch passes
    (130, {T.RMD_TUNE_SAMPLE_SPLIT: 1}),  # direct mode above 128 samples
]
MESH_FORMS = [
    (12, {}),  # split, one wave per item
    (12, {T.RMD_TUNE_SAMPLE_SPLIT: 1}),  # direct mode (the sum in memory)
    (12, {T.RMD_TUNE_SAMPLE_SPLIT: 1, T.RMD_TUNE_LAUNCH_FORM: 2}),
    (12, {T.RMD_TUNE_LAUNCH_FORM: 2}),  # persistent: path queues
    (12, {T.RMD_TUNE_LAUNCH_FORM: 2, T.RMD_TUNE_PATH_QUEUES: 1}),  # persistent lane-per-path, chained
    (12, {T.RMD_TUNE_LAUNCH_FORM: 2, T.RMD_TUNE_PATH_QUEUES: 1, T.RMD_TUNE_CHAIN_ITEMS: 1}),  # ... not chained
    (12, {T.RMD_TUNE_LAUNCH_FORM: 1, T.RMD_TUNE_SAMPLE_SPLIT: 2}),
    (40, {T.RMD_TUNE_SCRATCH_CAP_MB: 1}),  # several scratch passes
    (40, {T.RMD_TUNE_SCRATCH_CAP_MB: 1, T.RMD_TUNE_LAUNCH_FORM: 2}),
]


@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_moments_are_the_ordered_sum_of_squares_in_every_launch_form(gpu_ctx, which):
    sc = scenes.reflective_spheres() if which == "spheres" else scenes.gold_dragon_standin(n=12)
    forms = SPHERE_FORMS if which == "spheres" else MESH_FORMS
    tiles = generate_tiles(W, H, (32, 32))
    ds = render.DeviceScene(gpu_ctx, sc)
    fb, fb_sq = render.Framebuffer(gpu_ctx, W, H), render.Framebuffer(gpu_ctx, W, H)
    seen = []
    refs = {}
    try:
        for spp, tun in forms:
            st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=scenes.SEED)
            if spp not in refs:
                refs[spp] = ordered_sums(gpu_ctx, ds, st, spp)
            S_ref, Q_ref = refs[spp]
            fb.zero()
            plain = run_form(gpu_ctx, ds, st, tiles, tun, fb, None, with_sq=False)
            accum_plain = fb.download()
            fb.zero(), fb_sq.zero()
            mom = run_form(gpu_ctx, ds, st, tiles, tun, fb, fb_sq)
            assert mom == plain, "the moments launch took another form: %s vs %s" % (mom, plain)
            seen.append(dict(zip(INFO_FIELDS, mom)))
            assert fb.download().tobytes() == accum_plain.tobytes(), (spp, tun, mom)
            assert accum_plain.tobytes() == S_ref.tobytes(), "the probe's samples do not add up to the frame (%s)" % (tun,)
            assert fb_sq.download().tobytes() == Q_ref.tobytes(), (spp, tun, mom)
            assert (Q_ref > 0).any()
    finally:
        fb.close(), fb_sq.close(), ds.close()
    # the forms the comparison was meant to exercise were the ones launched
    assert {s["buffered"] for s in seen} == {0, 1} and {s["persistent"] for s in seen} == {0, 1}
    assert max(s["passes"] for s in seen) > 1 and {s["split_k"] > 1 for s in seen} == {False, True}
    if which == "mesh":
        assert {s["queued"] for s in seen} == {0, 1} and {s["chained"] for s in seen} == {0, 1}


@pytest.mark.parametrize("which,n,k", [("spheres", 130, 50), ("spheres", 12, 5), ("mesh", 12, 5)])
def test_moments_of_two_calls_equal_one_call(gpu_ctx, which, n, k):
    sc = scenes.reflective_spheres() if which == "spheres" else scenes.gold_dragon_standin(n=12)
    st = Settings(scenes.camera(W, H), sample_count=n, bounce_limit=5, seed=scenes.SEED + 3)
    tiles = generate_tiles(W, H, (32, 32))
    base = np.random.default_rng(1).uniform(0, 1, (H, W, 3))
    base_sq = np.random.default_rng(2).uniform(0, 1, (H, W, 3))
    ds = render.DeviceScene(gpu_ctx, sc)
    fb, fb_sq = render.Framebuffer(gpu_ctx, W, H), render.Framebuffer(gpu_ctx, W, H)
    try:
        fb.upload(base), fb_sq.upload(base_sq)
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb, 0, n, framebuffer_sq=fb_sq)
        one = fb.download(), fb_sq.download()
        fb.upload(base), fb_sq.upload(base_sq)
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb, 0, k, framebuffer_sq=fb_sq)
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb, k, n - k, framebuffer_sq=fb_sq)
        two = fb.download(), fb_sq.download()
        assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
        assert (one[1] != base_sq).any()
        # accum_sq = NULL through the moments entry point: rmd_render_tiles' frame and launch info
        fb.upload(base)
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb, 0, n)
        ref, ref_info = fb.download(), info_tuple(gpu_ctx)
        fb.upload(base)
        cam, pod = st.camera_settings.pod(), st.pod(0, n)
        import ctypes as C

        from raymond_amd.scene import tile_array

        gpu_ctx.check(gpu_ctx.L.rmd_render_tiles_moments(gpu_ctx.handle, ds.handle, C.byref(cam), C.byref(pod), tile_array(tiles), len(tiles), fb.ptr, None))
        assert fb.download().tobytes() == ref.tobytes() and info_tuple(gpu_ctx) == ref_info
        assert ref.tobytes() == one[0].tobytes()
    finally:
        fb.close(), fb_sq.close(), ds.close()


def numpy_tile_error(S, Q, n, floor, rect):
    l, t, w, h = rect
    s, q = S[t : t + h, l : l + w], Q[t : t + h, l : l + w]
    if s.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        m = s / float(n)
        v = (q - s * m) / (float(n) - 1.0)
        v = np.where(v < 0.0, 0.0, v)
        e = np.sqrt(v / float(n)) / np.maximum(np.abs(m), floor)
        ep = e.max(axis=2)
    bad = ~np.isfinite(s).all(axis=2) | ~np.isfinite(q).all(axis=2)
    if n < 2:
        bad[:] = True
    ep = np.where(bad, np.inf, ep)
    return float(ep.max())


def test_tile_error_matches_numpy(gpu_ctx):
    FW, FH = 96, 64
    rng = np.random.default_rng(11)
    n_max = 64
    L = rng.exponential(0.3, (n_max, FH, FW, 3)) * (rng.uniform(size=(n_max, FH, FW, 1)) < 0.7)
    rects = [(0, 0, 1, 1), (3, 2, 7, 5), (32, 0, 32, 32), (10, 10, 64, 48), (90, 60, 6, 4), (5, 5, 0, 3), (0, 0, FW, FH)]
    fb, fb_sq = render.Framebuffer(gpu_ctx, FW, FH), render.Framebuffer(gpu_ctx, FW, FH)
    try:
        for n in (1, 2, 7, 64):
            S = L[:n].sum(axis=0)
            Q = (L[:n] * L[:n]).sum(axis=0)
            S[0:4, 20:30] = 0.0  # black pixels: error 0
            Q[0:4, 20:30] = 0.0
            S[6, 4] = (3.0, 0.0, 1e-9)  # rounding below zero: clamped
            Q[6, 4] = (3.0 * 3.0 / n * (1.0 - 4e-16), 0.0, 1e-18 / n * (1.0 - 4e-16))
            S[12, 12, 1] = np.nan
            Q[20, 40, 2] = np.inf
            S[30, 70, 0] = -np.inf
            S[40, 50] = (1e-7, 2e-7, 5e-6)  # below the floor
            for floor in (1e-3, 0.25):
                fb.upload(S), fb_sq.upload(Q)
                got = render.tile_error(gpu_ctx, fb, fb_sq, n, floor, rects)
                want = np.array([numpy_tile_error(S, Q, n, floor, r) for r in rects])
                assert got.shape == want.shape
                fin = np.isfinite(want)
                assert (np.isfinite(got) == fin).all(), (n, floor, got, want)
                assert (got[~fin] == want[~fin]).all()
                np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12, atol=0)
                if n >= 2:
                    assert got[5] == 0.0  # no pixels
    finally:
        fb.close(), fb_sq.close()
    # a rect outside the frame is refused
    fb, fb_sq = render.Framebuffer(gpu_ctx, FW, FH), render.Framebuffer(gpu_ctx, FW, FH)
    try:
        with pytest.raises(Exception):
            render.tile_error(gpu_ctx, fb, fb_sq, 4, 1e-3, [(90, 0, 7, 1)])
    finally:
        fb.close(), fb_sq.close()


AW, AH, ASPP, ASPI = 96, 64, 64, 8


def uniform_reference(ctx, tile_size):
    """A uniform progressive render with moments: the frame and every tile's error after each pass of ASPI samples."""
    sc = scenes.reflective_spheres()
    st = Settings(scenes.camera(AW, AH), sample_count=ASPP, bounce_limit=5, seed=scenes.SEED, tile_size=tile_size)
    tiles = generate_tiles(AW, AH, tile_size)
    ds = render.DeviceScene(ctx, sc)
    fb, fb_sq = render.Framebuffer(ctx, AW, AH), render.Framebuffer(ctx, AW, AH)
    frames, errors = {}, {}
    try:
        for done in range(0, ASPP, ASPI):
            render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fb, done, ASPI, framebuffer_sq=fb_sq)
            c = done + ASPI
            frames[c] = fb.download()
            if c < ASPP:
                errors[c] = render.tile_error(ctx, fb, fb_sq, c, st.adaptive_floor, tiles)
    finally:
        fb.close(), fb_sq.close(), ds.close()
    return tiles, frames, errors


def pick_threshold(errors, n_tiles):
    """A threshold that some tiles reach at one of the checks and others at none of them."""
    best = np.min(np.stack([errors[c] for c in sorted(errors)]), axis=0)
    vals = np.unique(best)
    assert len(vals) >= 2
    thr = float(vals[len(vals) // 2 - 1] + vals[len(vals) // 2]) / 2.0
    early = [i for i in range(n_tiles) if best[i] <= thr]
    late = [i for i in range(n_tiles) if best[i] > thr]
    assert early and late
    return thr


def test_adaptive_render_tiled_finishes_converged_tiles_early(gpu_ctx):
    tiles, frames, errors = uniform_reference(gpu_ctx, (16, 16))
    thr = pick_threshold(errors, len(tiles))
    sc = scenes.reflective_spheres()
    st = Settings(scenes.camera(AW, AH), sample_count=ASPP, bounce_limit=5, seed=scenes.SEED, tile_size=(16, 16), samples_per_iteration=ASPI,
                  adaptive_threshold=thr)
    h = render.render_tiled(sc, st)
    msgs = list(h._messages)
    index = {t: i for i, t in enumerate(tiles)}
    finished = {}
    progressed = {i: [] for i in range(len(tiles))}
    for m in msgs:
        t = m.tile
        i = index[(t.left, t.top, t.width, t.height)]
        if m.kind == "TileFinished":
            assert i not in finished
            finished[i] = t
        else:
            progressed[i].append(t)
    assert sorted(finished) == list(range(len(tiles)))
    early = [i for i, t in finished.items() if t.sample_count < ASPP]
    full = [i for i, t in finished.items() if t.sample_count == ASPP]
    assert early and full
    for i, t in finished.items():
        l, tp, w, hh = tiles[i]
        c = t.sample_count
        # the sums of a uniform render at the tile's own count, bit for bit
        assert t.data.tobytes() == frames[c][tp : tp + hh, l : l + w].tobytes()
        checks = [c2 for c2 in sorted(errors) if c2 < c]
        assert [p.sample_count for p in progressed[i]] == checks
        for p in progressed[i]:  # every earlier check above the threshold
            assert p.error > thr and p.error == errors[p.sample_count][i]
            assert p.data.tobytes() == frames[p.sample_count][tp : tp + hh, l : l + w].tobytes()
        if c < ASPP:  # stopped at its first check at or below it
            assert t.error <= thr and t.error == errors[c][i]
        else:
            assert all(errors[c2][i] > thr for c2 in errors)
    # await divides each tile by its own count
    h2 = render.TaskHandle(st, msgs)
    h2.async_await()
    img = h2.await_()
    for i, t in finished.items():
        l, tp, w, hh = tiles[i]
        assert img[tp : tp + hh, l : l + w].tobytes() == (t.data / float(t.sample_count)).tobytes()


def test_adaptive_threshold_0_is_todays_render(gpu_ctx):
    tiles, frames, _ = uniform_reference(gpu_ctx, (16, 16))
    st = Settings(scenes.camera(AW, AH), sample_count=ASPP, bounce_limit=5, seed=scenes.SEED, tile_size=(16, 16), samples_per_iteration=ASPI,
                  adaptive_threshold=0.0)
    msgs = render.render_tiled(scenes.reflective_spheres(), st)._messages
    want = [("TileProgressed", r, c) for c in range(ASPI, ASPP, ASPI) for r in tiles] + [("TileFinished", r, ASPP) for r in tiles]
    got = [(m.kind, (m.tile.left, m.tile.top, m.tile.width, m.tile.height), m.tile.sample_count) for m in msgs]
    assert got == want
    for m in msgs:
        l, t, w, h = m.tile.left, m.tile.top, m.tile.width, m.tile.height
        assert m.tile.error is None
        assert m.tile.data.tobytes() == frames[m.tile.sample_count][t : t + h, l : l + w].tobytes()


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


@pytest.mark.parametrize("gpus", [1, 2])
def test_cpp_adaptive_render_equals_python(gpu_ctx, cli, tmp_path, gpus):
    tiles, frames, errors = uniform_reference(gpu_ctx, (32, 32))
    thr = pick_threshold(errors, len(tiles))
    raw = tmp_path / "o.f64"
    os.environ["RAYMOND_REHEARSE_ON_DEVICE0"] = "1"
    try:
        r = subprocess.run([cli, "render", "spheres", str(AW), str(AH), str(ASPP), "5", str(tmp_path / "o.ppm"), "--raw", str(raw), "--spi", str(ASPI),
                            "--gpus", str(gpus), "--adaptive", repr(thr)], capture_output=True, text=True)
    finally:
        os.environ.pop("RAYMOND_REHEARSE_ON_DEVICE0", None)
    assert r.returncode == 0, r.stderr
    img_cpp = np.fromfile(raw).reshape(AH, AW, 3)
    st = Settings(scenes.camera(AW, AH), sample_count=ASPP, bounce_limit=5, seed=scenes.SEED, tile_size=(32, 32), samples_per_iteration=ASPI,
                  adaptive_threshold=thr)
    h = render.render_tiled(scenes.reflective_spheres(), st)
    counts = sorted(m.tile.sample_count for m in h._messages if m.kind == "TileFinished")
    assert counts[0] < ASPP and counts[-1] == ASPP  # some tiles stopped early
    h.async_await()
    img_py = h.await_()
    assert img_cpp.tobytes() == img_py.tobytes()
