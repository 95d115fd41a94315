"""rmd_render_ids and rmd_ids_matte on the GPU, on the frames tests/test_gpu_features_scenes.py uses (tests/first_hit_ref.py: feature_keys), held to the
oracle exactly, in integers: the restatement tests/ids_ref.py applies the header's rule to the oracle's per-sample first-hit object.

  1  every case and every lens edge: the ten words of every pixel are the restatement's; at most 3 pixels a frame may leave through account_for_off_pixels
     below (the feature tests' own cap: the pixel re-run one sample per launch over a 1 x 1 rect, exactly one sample differs, its oracle hit fragile);
  2  the `other` path: table_edges-4 .. -7 (16 x 16, about 1,020 objects, 6 samples) have 21, 17, 18 and 15 pixels with other != 0 in the restatement,
     shuffled_room-1-aperture-4 13, -focal-1e6 3 (computed on the CPU from the oracle); the device's set of such pixels is the restatement's.  Under
     focal-negative and focal-nan every pixel is {key_0 = MISS, count_0 = samples};
  3  sample ranges add up, rect lists on and off the 8-pixel lattice agree, a pre-filled buffer keeps its words on uncovered pixels (and is continued on
     covered ones), the _async form followed by rmd_context_synchronize gives the same words;
  4  the object table at 511 / 512 objects (either side of launch_ids' dynamic-LDS opt-in) and at the 1,201 check_render_args accepts; one more is
     RMD_ERR_UNSUPPORTED from both forms with the buffer untouched; three_grids: a grid's key is the grid object's index + 1;
  5  rmd_ids_matte against the numpy matte bit for bit, other_pixels exactly, on the buffers of 1 and 2; alpha on open_scene-0;
  6  raymond_cli render --dump-ids / --dump-matte against the Python calls byte for byte.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import first_hit_ref as fr
import ids_ref
import oracle_lib as O
import test_gpu_features_scenes as fs
from raymond_amd import abi, probe, render, scenes
from raymond_amd.scene import CameraSettings, Settings, Transform, generate_tiles, tile_array
from test_gpu_sphere_scenes import rect_lists

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
MISS = ids_ref.MISS
KEYS = fr.feature_keys()
EDGE_KEYS = fr.feature_keys(lens_edges=True)
TABLE_KEYS = [("spheres", "table_edges", s, False, None) for s in (4, 5, 6, 7)]
OTHER_PIXELS = {**dict(zip(TABLE_KEYS, (21, 17, 18, 15))), ("spheres", "shuffled_room", 1, False, "aperture-4"): 13, ("spheres", "shuffled_room", 1, False, "focal-1e6"): 3}
NO_RAY_KEYS = [("spheres", "shuffled_room", 1, False, e) for e in ("focal-negative", "focal-nan")]
OPEN_SCENE = ("mesh", "open_scene", 0, False, None)
THREE_GRIDS = [k for k in KEYS if k[1] == "three_grids"]
RANGE_KEYS = [TABLE_KEYS[0], ("spheres", "camera_on_walls", 0, True, None), ("mesh", "camera_in_box", 1, True, None), ("mesh", "grid_positions", 2, False, None)] + THREE_GRIDS[:1]
MATTE_KEYS = TABLE_KEYS + [("spheres", "shuffled_room", 1, False, "aperture-4"), OPEN_SCENE] + THREE_GRIDS[:1]


@pytest.fixture(scope="module")
def ctx(product_lib):
    """A context of this module's own: the scenes are created under their cases' tunables."""
    with render.Context(0) as c:
        yield c


class Device(fs.Device):
    """One feature case's scene on the device (test_gpu_features_scenes.Device: created under the case's tunables) and its ID passes."""

    def __init__(self, ctx, fc):
        fs.Device.__init__(self, ctx, fc)
        self.ids = render.IdBuffer(ctx, self.W, self.H)
        self.open.append(self.ids)

    def run_ids(self, rects=None, ranges=None, base=None, sync=True):
        """-> (H, W, 10) words after the ID passes over `rects` (the frame in 32 x 32 tiles) and `ranges` (the case's samples) into a buffer that
        starts from `base` or zero"""
        st = self.fc.settings
        if base is None:
            self.ids.zero()
        else:
            self.ids.upload(base)
        for begin, count in ranges or [(self.fc.begin, self.fc.spp)]:
            render.render_ids(self.ctx, self.scene(), st.camera_settings, st, self.tiles if rects is None else rects, self.ids, begin, count, sync=sync)
        if not sync:
            self.ctx.synchronize()
        return self.ids.download()

    def sample_key(self, x, y, s):
        """the device's key of one sample: one launch over the 1 x 1 rect into a zeroed buffer"""
        rec = self.run_ids(rects=[(x, y, 1, 1)], ranges=[(s, 1)])[y, x]
        assert rec.tolist() == [int(rec[0]), 1, 0, 0, 0, 0, 0, 0, 0, 1] and rec[0] != 0, rec.tolist()
        return int(rec[0])


def account_for_off_pixels(dev, words, bad, label, limit=3):
    """first_hit_ref.account_for_off_pixels for ID words: every pixel in `bad` is traced again sample by sample and must be, word for word, the rule over
    those samples' keys; exactly ONE of its samples may have another key than the oracle's, and that sample's oracle hit must be fragile.  -> the number"""
    fc = dev.fc
    ys, xs = np.nonzero(bad)
    assert len(ys) <= limit, "%s: %d pixels differ from the restatement, first at (y, x) %s" % (label, len(ys), (int(ys[0]), int(xs[0])))
    osc = O.OracleScene(fc.scene)
    for y, x in zip(ys.tolist(), xs.tolist()):
        rec, off = np.zeros((1, 10), dtype=np.uint32), []
        for s in range(fc.begin, fc.begin + fc.spp):
            key = dev.sample_key(x, y, s)
            _, obj, t, sub, ok, rays = fr.sample_features(fc.scene, osc, fc.cam, fc.seed, fc.use_dof, [[x, y]], [s])
            if key != int(ids_ref.key_of(obj[0])):
                off.append((s, int(obj[0]), float(t[0]), int(sub[0]), rays[0]))
            ids_ref.insert(rec, np.array([key], dtype=np.uint32))
        assert rec[0].tolist() == words[y, x].tolist(), "%s: pixel (%d, %d) is not the rule over its samples" % (label, x, y)
        assert len(off) == 1, "%s: pixel (%d, %d) differs through %d samples: %s" % (label, x, y, len(off), [o[:4] for o in off])
        s, obj, t, sub, ray = off[0]
        why = fr.fragile_hit(fc.scene, osc, ray, obj, t, sub)
        print("%s: pixel (%d, %d) sample %d has another key: the oracle's hit (object %d, triangle %d, t %r) is %s" % (label, x, y, s, obj, sub, t, why))
        assert why is not None, "%s: pixel (%d, %d) sample %d differs from the oracle on a hit that is neither grazing nor tied" % (label, x, y, s)
    return len(ys)


_WORDS = {}


def device_words(ctx, key):
    """the device's words of a case, held to the restatement (1), computed once per process and shared read-only (2 and 5 read them)"""
    if key not in _WORDS:
        dev = Device(ctx, fr.feature_case(key))
        try:
            words = dev.run_ids()
            want = ids_ref.words_from_objs(fr.reference(key).objs)
            bad = (words != want).any(axis=2)
            entry = {"case": fr.feature_key_id(key), "pixels": int(bad.size), "pixels_that_differ": int(bad.sum()), "accounted_pixels": 0,
                     "pixels_with_other": int((words[..., 8] != 0).sum()), "used_slots_1_to_4": np.bincount(ids_ref.used_slots(words).ravel(), minlength=5)[1:].tolist()}
            try:
                if bad.any():
                    entry["accounted_pixels"] = account_for_off_pixels(dev, words, bad, entry["case"])
            finally:
                print("ids scenes: %s" % json.dumps(entry))  # the number accounted, per frame (pytest -s, or -rP, shows it)
            words.setflags(write=False)
            _WORDS[key] = (words, want, entry["accounted_pixels"])
        finally:
            dev.close()
    return _WORDS[key]


# ---------------------------------------------------------------- 1
@pytest.mark.parametrize("key", KEYS + EDGE_KEYS, ids=fs.ids(KEYS + EDGE_KEYS))
def test_every_case_and_lens_edge_is_the_restatement_word_for_word(ctx, oracle, key):
    words, want, accounted = device_words(ctx, key)
    assert words.shape == want.shape == fr.reference(key).objs.shape[1:] + (10,) and words.dtype == np.uint32
    assert accounted <= 3
    w = words.astype(np.uint64)
    assert (w[..., 1:8:2].sum(axis=-1) + w[..., 8] == w[..., 9]).all() and (w[..., 9] == fr.FEATURE_SPP).all()  # sum + other == samples


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("key", list(OTHER_PIXELS), ids=fs.ids(list(OTHER_PIXELS)))
def test_the_other_path(ctx, oracle, key):
    words, want, _ = device_words(ctx, key)
    assert int((want[..., 8] != 0).sum()) == OTHER_PIXELS[key]  # 5 or 6 distinct first hits in 6 samples
    assert ((words[..., 8] != 0) == (want[..., 8] != 0)).all() and (words[want[..., 8] != 0] == want[want[..., 8] != 0]).all()
    over = words[words[..., 8] != 0]
    assert (over[:, 0:8:2] != 0).all() and set(over[:, 8].tolist()) <= {1, 2}


@pytest.mark.parametrize("key", NO_RAY_KEYS, ids=fs.ids(NO_RAY_KEYS))
def test_no_sample_has_a_ray_every_pixel_is_the_miss(ctx, oracle, key):
    words, _, accounted = device_words(ctx, key)
    assert accounted == 0 and (words == np.array([MISS, fr.FEATURE_SPP, 0, 0, 0, 0, 0, 0, 0, fr.FEATURE_SPP], dtype=np.uint32)).all()


# ---------------------------------------------------------------- 3
def prefill(key, W, H, n_objects):
    """reachable records over the scene's own objects (two samples of the rule), so that the pass continues tables that hold its keys"""
    rng = np.random.default_rng([key[2], int(key[3]), len(key[1]), 34])
    return ids_ref.words_from_objs(rng.integers(-1, min(n_objects, 12), (2, H, W)))


@pytest.mark.parametrize("key", RANGE_KEYS, ids=fs.ids(RANGE_KEYS))
def test_sample_ranges_rect_lists_uncovered_pixels_and_the_async_form(ctx, oracle, key):
    fc = fr.feature_case(key)
    _, _, accounted = device_words(ctx, key)
    dev = Device(ctx, fc)
    try:
        W, H, b, n = dev.W, dev.H, fc.begin, fc.spp
        base = prefill(key, W, H, len(fc.scene.objects))
        full = [(0, 0, W, H)]
        one = dev.run_ids(rects=full, base=base)
        if accounted == 0:  # (held to the oracle from zero: here the same samples continue the pre-fill's tables)
            assert one.tobytes() == ids_ref.words_from_objs(fr.reference(key).objs, base=base).tobytes()
        assert (one[..., 9] == base[..., 9] + n).all() and one.tobytes() != dev.run_ids(rects=full).tobytes()
        # [0, k) then [k, n) == [0, n), for every k
        for k in range(0, n + 1):
            assert dev.run_ids(rects=full, ranges=[(b, k), (b + k, n - k)], base=base).tobytes() == one.tobytes(), k
        # one rect == 8 x 8 tiles == 5 x 3 tiles == 32 x 32 tiles
        for ts in ((8, 8), (5, 3), (32, 32)):
            assert dev.run_ids(rects=generate_tiles(W, H, ts), base=base).tobytes() == one.tobytes(), ts
        # rect lists off the 8-pixel lattice: covered pixels agree, the others keep the pre-fill's words
        for rects in rect_lists(W, H):
            covered = np.zeros((H, W), dtype=bool)
            for (l, t, w, h) in rects:
                assert w > 0 and h > 0 and l + w <= W and t + h <= H and not covered[t : t + h, l : l + w].any()
                covered[t : t + h, l : l + w] = True
            assert covered.any() and not covered.all()
            got = dev.run_ids(rects=rects, base=base)
            assert got[covered].tobytes() == one[covered].tobytes() and got[~covered].tobytes() == base[~covered].tobytes(), rects[:2]
        # the _async form, then rmd_context_synchronize
        assert dev.run_ids(rects=full, ranges=[(b, 2), (b + 2, n - 2)], base=base, sync=False).tobytes() == one.tobytes()
    finally:
        dev.close()


# ---------------------------------------------------------------- 4
def check_table(ctx, sc, label, accepted):
    W, H, spp, seed = 16, 16, 4, 0x7AB1E
    cam = CameraSettings(W, H, 55.0, Transform((0.0, 0.0, 0.0)))
    fc = fr.FeatureCase(None, sc, cam, Settings(cam, sample_count=spp, bounce_limit=1, seed=seed), seed, False, 0, spp, {})
    dev = Device(ctx, fc)
    try:
        ds = dev.scene()
        n = probe.scene_layout(ds)[0]
        if accepted:
            words = dev.run_ids()
            objs = fr.first_hit_sums(sc, cam, seed, spp)[2]
            want = ids_ref.words_from_objs(objs)
            bad = (words != want).any(axis=2)
            accounted = account_for_off_pixels(dev, words, bad, label) if bad.any() else 0
            print("ids scenes: %s" % json.dumps({"case": label, "pixels": W * H, "pixels_that_differ": int(bad.sum()), "accounted_pixels": accounted, "objects": n,
                                                  "distinct_first_hits": int(len(np.unique(objs))), "pixels_with_other": int((words[..., 8] != 0).sum())}))
            assert len(np.unique(objs)) > 10 and int(words[..., 0:8:2].max()) > 256  # the table's spheres are seen, with keys past the first 256 objects
            return n
        base = prefill(("", "", n, False, None), W, H, n)
        dev.ids.upload(base)
        c, s, rects = cam.pod(), fc.settings.pod(0, spp), tile_array([(0, 0, W, H)])
        for fn in (ctx.L.rmd_render_ids, ctx.L.rmd_render_ids_async):
            assert fn(ctx.handle, ds.handle, C.byref(c), C.byref(s), rects, 1, dev.ids.ptr) == abi.RMD_ERR_UNSUPPORTED, label
        ctx.synchronize()
        assert dev.ids.download().tobytes() == base.tobytes()
        return n
    finally:
        dev.close()


def test_the_object_table_at_the_lds_edges(ctx, oracle):
    tiles, buffered = probe.launch_sizes(probe.MODE_TILES, False), probe.launch_sizes(probe.MODE_TILES_BUFFERED, False)
    below = (64 * 1024 - tiles["wave"]) // tiles["object"]  # launch_ids' plan, one wave per item: the last table without the dynamic-LDS opt-in
    largest = (tiles["budget"] - buffered["wave"]) // tiles["object"]  # check_render_args: the table beside one wave's area and the sort pool
    assert (below, largest) == (511, 1201)
    for n, label, accepted in ((below, "at the opt-in", True), (below + 1, "past the opt-in", True), (largest, "largest table", True), (largest + 1, "one more", False)):
        assert check_table(ctx, fs.table_scene(n), "object table %s: %d objects" % (label, n), accepted) == n


@pytest.mark.parametrize("key", THREE_GRIDS, ids=fs.ids(THREE_GRIDS))
def test_a_grids_key_is_the_grid_objects_index(ctx, oracle, key):
    words, want, _ = device_words(ctx, key)
    fc = fr.feature_case(key)
    grid_keys = [i + 1 for i, o in enumerate(fc.scene.flatten()[0][: len(fc.scene.objects)]) if o.geometry_kind == 2]
    assert len(grid_keys) == 3
    seen = set(np.unique(words[..., 0:8:2]).tolist())
    assert seen == set(np.unique(want[..., 0:8:2]).tolist()) and seen & set(grid_keys), (sorted(seen), grid_keys)
    assert seen - {0, MISS} <= set(range(1, len(fc.scene.objects) + 1))


# ---------------------------------------------------------------- 5
def object_lists(words, n_objects):
    """the cases: one object, several, with miss, the empty list, a list naming no object of the frame, duplicates"""
    keys, counts = np.unique(words[..., 0:8:2], return_counts=True)
    seen = [int(k) - 1 for k in keys[np.argsort(-counts)] if k not in (0, MISS)]
    unseen = [o for o in range(n_objects + 5) if o not in seen][:3] + [n_objects + 1000]
    return {"one": seen[:1], "several": seen[:3] + seen[-2:], "with_miss": seen[1:3] + [MISS], "miss": [MISS], "empty": [], "unseen": unseen,
            "duplicates": seen[:2] * 3 + [MISS, MISS] + seen[:1], "many": list(range(min(n_objects, 2047))) + [MISS]}


@pytest.mark.parametrize("key", MATTE_KEYS, ids=fs.ids(MATTE_KEYS))
def test_the_matte_is_the_numpy_matte_bit_for_bit(ctx, oracle, key):
    words, _, _ = device_words(ctx, key)
    fc = fr.feature_case(key)
    H, W = words.shape[:2]
    with render.IdBuffer(ctx, W, H) as ids:
        ids.upload(words)
        between = False
        for name, objects in object_lists(words, len(fc.scene.objects)).items():
            got, other = render.ids_matte(ctx, ids, objects)
            want, want_other = ids_ref.matte(words, objects)
            assert got.shape == (H, W) and got.tobytes() == want.tobytes() and other == want_other == OTHER_PIXELS.get(key, other), name
            between |= bool(((got > 0) & (got < 1)).any())
            if name in ("empty", "unseen"):
                assert not got.any()
            if name == "many" and key not in OTHER_PIXELS:
                assert (got == 1.0).all()  # every object and the miss, no overflow: the whole pixel
        assert between
        ids.zero()  # a zeroed buffer: samples == 0 everywhere
        got, other = render.ids_matte(ctx, ids, [0, MISS])
        assert got.tobytes() == np.zeros((H, W)).tobytes() and other == 0


def test_alpha_of_an_open_scene(ctx, oracle):
    words, _, accounted = device_words(ctx, OPEN_SCENE)
    objs = fr.reference(OPEN_SCENE).objs
    H, W = words.shape[:2]
    with render.IdBuffer(ctx, W, H) as ids:
        ids.upload(words)
        matte, other = render.ids_matte(ctx, ids, [MISS])
    alpha = 1.0 - matte
    assert other == 0 and (alpha > 0).any() and (alpha < 1).any() and ((alpha > 0) & (alpha < 1)).any()
    if accounted == 0:
        missed = (objs < 0).sum(axis=0).astype(np.float64)
        assert alpha.tobytes() == (1.0 - missed / fr.FEATURE_SPP).tobytes()
        assert np.abs(alpha - (objs >= 0).mean(axis=0)).max() <= 2.0 ** -52  # the share of samples that show an object


# ---------------------------------------------------------------- 6
def test_cli_dump_ids_and_dump_matte_equal_the_python_calls(ctx, tmp_path):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    W, H, spp, bounces = 64, 48, 4, 2
    ids_file, matte_file = tmp_path / "ids.u32", tmp_path / "matte.f64"
    r = subprocess.run([CLI, "render", "spheres", str(W), str(H), str(spp), str(bounces), str(tmp_path / "o.ppm"), "--dump-ids", str(ids_file), "--dump-matte", str(matte_file),
                        "--matte-objects", "0,3,miss,3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sc = scenes.reflective_spheres()
    st = Settings(scenes.camera(W, H), sample_count=spp, tile_size=(32, 32), bounce_limit=bounces, seed=scenes.SEED)
    rects = generate_tiles(W, H, (32, 32))
    words = render.render_ids_arrays(ctx, sc, st, rects, [spp] * len(rects))
    assert words.shape == (H, W, 10) and (words[..., 9] == spp).all() and len(np.unique(words[..., 0])) > 3
    assert ids_file.read_bytes() == words.astype("<u4").tobytes()
    with render.IdBuffer(ctx, W, H) as ids:
        ids.upload(words)
        matte, other = render.ids_matte(ctx, ids, [0, 3, MISS, 3])
    assert matte_file.read_bytes() == matte.tobytes() and matte.any()
    assert "matte: %d pixels with other != 0" % other in r.stdout
    keys, counts = render.ids_ranked(words)
    assert (counts[..., 0] >= counts[..., 1]).all() and (keys[..., 0] != 0).all()
