"""rmd_render_ao and rmd_ao_resolve on the GPU, on the frames tests/test_gpu_features_scenes.py uses (tests/first_hit_ref.py: feature_keys), held to the
oracle exactly, in integers: the restatement tests/ao_ref.py composes each sample's bounce ray from the oracle's entry points and counts it.

  1  every case and every lens edge at its max_distance (ao_ref.case_distance: 1.0): the four words of every pixel are the restatement's; at most 3
     pixels a frame may leave through account_for_off_pixels below (the feature tests' own cap: the pixel re-run one sample per launch over a 1 x 1
     rect, the pixel the sum of those, exactly one sample differs, and that sample fragile — ao_ref.fragile_sample; tests/test_ao_host.py holds the
     frames to the cap); occluded + open + none == samples everywhere;
  2  max_distance = +inf on open_scene-0 and on a closed room, 1e-3 on the room (ao_ref.EXTRA_DISTANCES): a pixel's occluded count does not fall as
     the distance grows; nan_normals: a NaN normal makes a NaN ray, which hits nothing and counts as open;
  3  sample ranges add up at every split point, rect lists on and off the 8-pixel lattice agree, a pre-filled buffer keeps its words on uncovered
     pixels (and is continued on covered ones), the _async form followed by rmd_context_synchronize gives the same words;
  4  the object table at 511 / 512 objects (either side of the launch's dynamic-LDS opt-in) and at the 1,201 check_render_args accepts; one more is
     RMD_ERR_UNSUPPORTED from both forms with the buffer untouched; three_grids: bounce rays that end on each of the grids;
  5  rmd_ao_resolve against the numpy resolve bit for bit, empty_pixels exactly;
  6  raymond_cli render --dump-ao against the Python calls byte for byte.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import ao_ref
import first_hit_ref as fr
import oracle_lib as O
import test_gpu_features_scenes as fs
from raymond_amd import abi, probe, render, scenes
from raymond_amd.scene import CameraSettings, Settings, Transform, generate_tiles, tile_array
from test_gpu_sphere_scenes import rect_lists

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
KEYS = fr.feature_keys()
EDGE_KEYS = fr.feature_keys(lens_edges=True)
INF = float("inf")
OPEN_SCENE, ROOM = ao_ref.OPEN_SCENE, ao_ref.ROOM
NAN_NORMALS = [k for k in KEYS if k[1] == "nan_normals"]
THREE_GRIDS = [k for k in KEYS if k[1] == "three_grids"]
NO_RAY_KEYS = [("spheres", "shuffled_room", 1, False, e) for e in ("focal-negative", "focal-nan")]
RANGE_KEYS = [("spheres", "table_edges", 4, False, None), ("spheres", "camera_on_walls", 0, True, None), ("mesh", "camera_in_box", 1, True, None),
              ("mesh", "grid_positions", 2, False, None)] + THREE_GRIDS[:1]
RESOLVE_KEYS = [OPEN_SCENE, ROOM, ("spheres", "shuffled_room", 1, False, "aperture-4"), ("spheres", "shuffled_room", 1, False, "focal-negative")] + THREE_GRIDS[:1]


@pytest.fixture(scope="module")
def ctx(product_lib):
    """A context of this module's own: the scenes are created under their cases' tunables."""
    with render.Context(0) as c:
        yield c


class Device(fs.Device):
    """One feature case's scene on the device (test_gpu_features_scenes.Device: created under the case's tunables) and its AO passes."""

    def __init__(self, ctx, fc):
        fs.Device.__init__(self, ctx, fc)
        self.ao = render.AoBuffer(ctx, self.W, self.H)
        self.open.append(self.ao)

    def run_ao(self, D, rects=None, ranges=None, base=None, sync=True):
        """-> (H, W, 4) words after the AO passes at max_distance D over `rects` (the frame in 32 x 32 tiles) and `ranges` (the case's samples) into a
        buffer that starts from `base` or zero"""
        st = self.fc.settings
        if base is None:
            self.ao.zero()
        else:
            self.ao.upload(base)
        for begin, count in ranges or [(self.fc.begin, self.fc.spp)]:
            render.render_ao(self.ctx, self.scene(), st.camera_settings, st, self.tiles if rects is None else rects, D, self.ao, begin, count, sync=sync)
        if not sync:
            self.ctx.synchronize()
        return self.ao.download()

    def sample_words(self, x, y, s, D):
        """the device's record of one sample: one launch over the 1 x 1 rect into a zeroed buffer"""
        rec = self.run_ao(D, rects=[(x, y, 1, 1)], ranges=[(s, 1)])[y, x]
        assert rec[3] == 1 and sorted(rec[:3].tolist()) == [0, 0, 1], rec.tolist()
        return rec


def account_for_off_pixels(dev, words, bad, D, label, limit=3):
    """first_hit_ref.account_for_off_pixels for AO words: every pixel in `bad` is traced again sample by sample and must be, word for word, the sum of
    those samples' records; exactly ONE of its samples may have another record than the restatement's, and that sample must be fragile.  -> the number"""
    fc = dev.fc
    ys, xs = np.nonzero(bad)
    assert len(ys) <= limit, "%s: %d pixels differ from the restatement, first at (y, x) %s" % (label, len(ys), (int(ys[0]), int(xs[0])))
    osc = O.OracleScene(fc.scene)
    for y, x in zip(ys.tolist(), xs.tolist()):
        rec, off = np.zeros(4, dtype=np.uint32), []
        for s in range(fc.begin, fc.begin + fc.spp):
            got = dev.sample_words(x, y, s, D)
            S = ao_ref.sample_ao(fc.scene, osc, fc.cam, fc.seed, fc.use_dof, [[x, y]], [s], D)
            want = np.zeros((1, 4), dtype=np.uint32)
            ao_ref.count(want, S.first, S.occluded)
            if got.tolist() != want[0].tolist():
                off.append((s, S))
            rec = rec + got
        assert rec.tolist() == words[y, x].tolist(), "%s: pixel (%d, %d) is not the sum of its samples" % (label, x, y)
        assert len(off) == 1, "%s: pixel (%d, %d) differs through %d samples: %s" % (label, x, y, len(off), [o[0] for o in off])
        s, S = off[0]
        why = ao_ref.fragile_sample(fc.scene, osc, S, D)
        print("%s: pixel (%d, %d) sample %d has another outcome: the restatement's (first hit object %d, t %r; the bounce's object %d, t2 %r) is %s"
              % (label, x, y, s, int(S.obj[0]), float(S.t[0]), int(S.obj2[0]), float(S.t2[0]), why))
        assert why is not None, "%s: pixel (%d, %d) sample %d differs from the restatement on a sample that is not fragile" % (label, x, y, s)
    return len(ys)


_WORDS = {}


def device_words(ctx, key, D=None):
    """the device's words of a case at max_distance D (None: the case's own), held to the restatement (1), computed once per process and shared
    read-only -> (words, the restatement's words, the pixels accounted as fragile)"""
    D = ao_ref.case_distance(key) if D is None else D
    if (key, D) not in _WORDS:
        dev = Device(ctx, fr.feature_case(key))
        try:
            words = dev.run_ao(D)
            want = ao_ref.reference(key, D)[1]
            bad = (words != want).any(axis=2)
            entry = {"case": fr.feature_key_id(key), "max_distance": repr(D), "pixels": int(bad.size), "pixels_that_differ": int(bad.sum()), "accounted_pixels": 0,
                     "occluded": int(words[..., 0].sum()), "open": int(words[..., 1].sum()), "none": int(words[..., 2].sum())}
            try:
                if bad.any():
                    entry["accounted_pixels"] = account_for_off_pixels(dev, words, bad, D, entry["case"])
            finally:
                print("ao scenes: %s" % json.dumps(entry))  # the number accounted, per frame (pytest -s, or -rP, shows it)
            words.setflags(write=False)
            _WORDS[(key, D)] = (words, want, entry["accounted_pixels"])
        finally:
            dev.close()
    return _WORDS[(key, D)]


def adds_up(words, spp):
    w = words.astype(np.uint64)
    return bool((w[..., 0] + w[..., 1] + w[..., 2] == w[..., 3]).all() and (w[..., 3] == spp).all())


# ---------------------------------------------------------------- 1
@pytest.mark.parametrize("key", KEYS + EDGE_KEYS, ids=fs.ids(KEYS + EDGE_KEYS))
def test_every_case_and_lens_edge_is_the_restatement_word_for_word(ctx, oracle, key):
    words, want, accounted = device_words(ctx, key)
    assert words.shape == want.shape == ao_ref.reference(key)[0].first.shape[1:] + (4,) and words.dtype == np.uint32
    assert accounted <= 3 and adds_up(words, fr.FEATURE_SPP)


@pytest.mark.parametrize("key", NO_RAY_KEYS, ids=fs.ids(NO_RAY_KEYS))
def test_no_sample_has_a_ray_every_pixel_is_none(ctx, oracle, key):
    words, _, accounted = device_words(ctx, key)
    assert accounted == 0 and (words == np.array([0, 0, fr.FEATURE_SPP, fr.FEATURE_SPP], dtype=np.uint32)).all()


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("key,D", ao_ref.EXTRA_DISTANCES, ids=["%s-%r" % (fr.feature_key_id(k), d) for k, d in ao_ref.EXTRA_DISTANCES])
def test_the_distance_at_its_ends(ctx, oracle, key, D):
    words, want, accounted = device_words(ctx, key, D)
    usual, _, accounted_usual = device_words(ctx, key)
    assert accounted <= 3 and adds_up(words, fr.FEATURE_SPP) and (words[..., 2] == usual[..., 2]).all()  # the first hits do not depend on the distance
    S = ao_ref.reference(key, D)[0]
    if accounted == 0 and accounted_usual == 0:
        lo, hi = (words, usual) if D < ao_ref.case_distance(key) else (usual, words)
        assert (lo[..., 0] <= hi[..., 0]).all() and (lo[..., 0] < hi[..., 0]).any()  # occluded does not fall as the distance grows, and here it moves
    if D == INF:  # any hit: open is exactly the bounce rays that hit nothing
        assert (want[..., 1] == (S.first & (S.obj2 < 0)).sum(axis=0)).all()
        assert (want[..., 1] != 0).any() == (key == OPEN_SCENE)  # a closed room lets no ray out
    else:
        assert want[..., 0].sum() < want[..., 1].sum() // 20  # almost nothing lies within 1e-3 of a surface point


@pytest.mark.parametrize("key", NAN_NORMALS, ids=fs.ids(NAN_NORMALS))
def test_a_nan_normal_counts_as_open(ctx, oracle, key):
    words, want, accounted = device_words(ctx, key)
    S = ao_ref.reference(key)[0]
    nan_ray = S.first & np.isnan(S.rays2).any(axis=-1)
    assert not (S.occluded & nan_ray).any() and (S.obj2[nan_ray] < 0).all()
    if key == NAN_NORMALS[-1]:
        assert nan_ray.sum() > 100  # (nan_normals-1: 156 of its 7,128 first hits)
    if accounted == 0:
        assert (words[..., 1] >= nan_ray.sum(axis=0)).all()


# ---------------------------------------------------------------- 3
def prefill(key, W, H):
    """records that hold counts already (sums of three counts), so that the pass continues them"""
    rng = np.random.default_rng([key[2], int(key[3]), len(key[1]), 35])
    base = np.zeros((H, W, 4), dtype=np.uint32)
    base[..., :3] = rng.integers(0, 9, (H, W, 3))
    base[0, 0, :3] = 0xFFFFFFFF  # counts are modulo 2^32
    base[..., 3] = base[..., 0] + base[..., 1] + base[..., 2]
    return base


@pytest.mark.parametrize("key", RANGE_KEYS, ids=fs.ids(RANGE_KEYS))
def test_sample_ranges_rect_lists_uncovered_pixels_and_the_async_form(ctx, oracle, key):
    fc = fr.feature_case(key)
    D = ao_ref.case_distance(key)
    words, _, accounted = device_words(ctx, key)
    dev = Device(ctx, fc)
    try:
        W, H, b, n = dev.W, dev.H, fc.begin, fc.spp
        base = prefill(key, W, H)
        full = [(0, 0, W, H)]
        one = dev.run_ao(D, rects=full, base=base)
        assert one.tobytes() == (base + words).tobytes() and one.tobytes() != words.tobytes()  # the pre-fill continued, modulo 2^32
        if accounted == 0:
            S = ao_ref.reference(key)[0]
            assert one.tobytes() == ao_ref.words_from_samples(S.first, S.occluded, base=base).tobytes()
        # [0, k) then [k, n) == [0, n), for every k
        for k in range(0, n + 1):
            assert dev.run_ao(D, rects=full, ranges=[(b, k), (b + k, n - k)], base=base).tobytes() == one.tobytes(), k
        # one rect == 8 x 8 tiles == 5 x 3 tiles == 32 x 32 tiles
        for ts in ((8, 8), (5, 3), (32, 32)):
            assert dev.run_ao(D, rects=generate_tiles(W, H, ts), base=base).tobytes() == one.tobytes(), ts
        # rect lists off the 8-pixel lattice: covered pixels agree, the others keep the pre-fill's words
        for rects in rect_lists(W, H):
            covered = np.zeros((H, W), dtype=bool)
            for (l, t, w, h) in rects:
                assert w > 0 and h > 0 and l + w <= W and t + h <= H and not covered[t : t + h, l : l + w].any()
                covered[t : t + h, l : l + w] = True
            assert covered.any() and not covered.all()
            got = dev.run_ao(D, rects=rects, base=base)
            assert got[covered].tobytes() == one[covered].tobytes() and got[~covered].tobytes() == base[~covered].tobytes(), rects[:2]
        # the _async form, then rmd_context_synchronize
        assert dev.run_ao(D, rects=full, ranges=[(b, 2), (b + 2, n - 2)], base=base, sync=False).tobytes() == one.tobytes()
    finally:
        dev.close()


# ---------------------------------------------------------------- 4
def check_table(ctx, sc, label, accepted):
    W, H, spp, seed, D = 16, 16, 4, 0x7AB1E, 1.0
    cam = CameraSettings(W, H, 55.0, Transform((0.0, 0.0, 0.0)))
    fc = fr.FeatureCase(None, sc, cam, Settings(cam, sample_count=spp, bounce_limit=1, seed=seed), seed, False, 0, spp, {})
    dev = Device(ctx, fc)
    try:
        ds = dev.scene()
        n = probe.scene_layout(ds)[0]
        if accepted:
            words = dev.run_ao(D)
            S = ao_ref.frame_samples(sc, cam, seed, spp, 0, False, D)
            want = ao_ref.words_from_samples(S.first, S.occluded)
            bad = (words != want).any(axis=2)
            accounted = account_for_off_pixels(dev, words, bad, D, label) if bad.any() else 0
            print("ao scenes: %s" % json.dumps({"case": label, "pixels": W * H, "pixels_that_differ": int(bad.sum()), "accounted_pixels": accounted, "objects": n,
                                                 "distinct_occluders": int(len(np.unique(S.obj2[S.occluded]))), "occluded": int(words[..., 0].sum())}))
            assert adds_up(words, spp) and len(np.unique(S.obj2[S.occluded])) > 10 and int(S.obj2.max()) > 256  # the table's spheres occlude, past the first 256 objects
            return n
        base = prefill(("", "", n, False, None), W, H)
        dev.ao.upload(base)
        c, s, rects = cam.pod(), fc.settings.pod(0, spp), tile_array([(0, 0, W, H)])
        for fn in (ctx.L.rmd_render_ao, ctx.L.rmd_render_ao_async):
            assert fn(ctx.handle, ds.handle, C.byref(c), C.byref(s), rects, 1, D, dev.ao.ptr) == abi.RMD_ERR_UNSUPPORTED, label
        ctx.synchronize()
        assert dev.ao.download().tobytes() == base.tobytes()
        return n
    finally:
        dev.close()


def test_the_object_table_at_the_lds_edges(ctx, oracle):
    tiles, buffered = probe.launch_sizes(probe.MODE_TILES, False), probe.launch_sizes(probe.MODE_TILES_BUFFERED, False)
    below = (64 * 1024 - tiles["wave"]) // tiles["object"]  # the launch's plan, one wave per item: the last table without the dynamic-LDS opt-in
    largest = (tiles["budget"] - buffered["wave"]) // tiles["object"]  # check_render_args: the table beside one wave's area and the sort pool
    assert (below, largest) == (511, 1201)
    for n, label, accepted in ((below, "at the opt-in", True), (below + 1, "past the opt-in", True), (largest, "largest table", True), (largest + 1, "one more", False)):
        assert check_table(ctx, fs.table_scene(n), "object table %s: %d objects" % (label, n), accepted) == n


@pytest.mark.parametrize("key", THREE_GRIDS, ids=fs.ids(THREE_GRIDS))
def test_bounce_rays_end_on_each_of_three_grids(ctx, oracle, key):
    words, want, accounted = device_words(ctx, key)
    fc = fr.feature_case(key)
    S = ao_ref.reference(key)[0]
    grids = [i for i, o in enumerate(fc.scene.flatten()[0][: len(fc.scene.objects)]) if o.geometry_kind == 2]
    assert len(grids) == 3 and accounted <= 3
    assert set(grids) <= set(np.unique(S.obj2[S.occluded]).tolist())  # every grid occludes some sample of the frame, and the words are the restatement's (1)


# ---------------------------------------------------------------- 5
@pytest.mark.parametrize("key", RESOLVE_KEYS, ids=fs.ids(RESOLVE_KEYS))
def test_the_resolve_is_the_numpy_resolve_bit_for_bit(ctx, oracle, key):
    words, _, _ = device_words(ctx, key)
    H, W = words.shape[:2]
    with render.AoBuffer(ctx, W, H) as ao:
        ao.upload(words)
        for empty_value in (1.0, 0.0, -2.5):
            got, empty = render.ao_resolve(ctx, ao, empty_value)
            want, want_empty = ao_ref.resolve(words, empty_value)
            assert got.shape == (H, W) and got.tobytes() == want.tobytes() and empty == want_empty == int(((words[..., 0] == 0) & (words[..., 1] == 0)).sum())
        if key == OPEN_SCENE:
            assert 0 < empty < W * H  # pixels that see only the background
        if key[4] == "focal-negative":
            assert empty == W * H
        random = ao_ref.random_records(np.random.default_rng(W * H), W * H).reshape(H, W, 4)  # counts past 2^31, sums past 2^32, zero denominators
        ao.upload(random)
        got, empty = render.ao_resolve(ctx, ao, 0.5)
        want, want_empty = ao_ref.resolve(random, 0.5)
        assert got.tobytes() == want.tobytes() and empty == want_empty and ((got > 0) & (got < 1)).any()
        ao.zero()  # a zeroed buffer: every pixel is empty
        got, empty = render.ao_resolve(ctx, ao)
        assert got.tobytes() == np.ones((H, W)).tobytes() and empty == W * H


def test_the_resolve_counts_across_waves_and_blocks(ctx):
    W, H = 301, 67  # no multiple of the wave or the block: several blocks, a last wave that is part empty
    words = ao_ref.random_records(np.random.default_rng(7), W * H).reshape(H, W, 4)
    with render.AoBuffer(ctx, W, H) as ao:
        ao.upload(words)
        got, empty = render.ao_resolve(ctx, ao, 0.75)
        want, want_empty = ao_ref.resolve(words, 0.75)
        assert got.tobytes() == want.tobytes() and empty == want_empty and 0 < empty < W * H
        assert render.ao_resolve(ctx, ao, 0.75)[1] == want_empty  # the context's counter starts from zero again


# ---------------------------------------------------------------- 6
def test_cli_dump_ao_equals_the_python_calls(ctx, tmp_path):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    W, H, spp, bounces = 64, 48, 4, 2
    ao_file = tmp_path / "ao.f64"
    r = subprocess.run([CLI, "render", "spheres", str(W), str(H), str(spp), str(bounces), str(tmp_path / "o.ppm"), "--dump-ao", str(ao_file), "--ao-distance", "0.75", "--ao-empty", "0.25"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sc = scenes.reflective_spheres()
    st = Settings(scenes.camera(W, H), sample_count=spp, tile_size=(32, 32), bounce_limit=bounces, seed=scenes.SEED)
    rects = generate_tiles(W, H, (32, 32))
    words = render.render_ao_arrays(ctx, sc, st, rects, [spp] * len(rects), 0.75)
    assert words.shape == (H, W, 4) and adds_up(words, spp) and words[..., 0].any() and words[..., 1].any()
    with render.AoBuffer(ctx, W, H) as ao:
        ao.upload(words)
        image, empty = render.ao_resolve(ctx, ao, 0.25)
    assert ao_file.read_bytes() == image.tobytes() and ((image > 0) & (image < 1)).any()
    assert "ao: %d pixels without a first hit" % empty in r.stdout
    r = subprocess.run([CLI, "render", "spheres", str(W), str(H), str(spp), str(bounces), str(tmp_path / "o.ppm"), "--dump-ao", str(ao_file)], capture_output=True, text=True)
    assert r.returncode != 0 and "--ao-distance" in r.stderr  # the distance has no default
