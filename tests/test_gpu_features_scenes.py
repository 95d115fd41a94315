"""rmd_render_features on the adversarial scenes of tests/sphere_scenes.py and tests/mesh_scenes.py, and under adversarial lenses, on the GPU.

The feature kernel (features.hip: features_kernel<GRID>) calls the machinery the render kernels call — scene_intersect_wave with the launch's axis
pairs and visit mask, the LDS-staged object table, the wave-cooperative walk, the thin lens — with its own arguments; tests/test_gpu_features.py
sees it on the stock room with the stock camera.  Here, at the classes' own frames, 6 samples a pixel (from sample 5 on odd seeds), the scene
created under mesh_scenes.scene_tunables:

  a  every case, the thin-lens variants with use_dof and the class's aperture, against the oracle's composition (tests/first_hit_ref.py, which
     tests/test_first_hit_host.py ties to the oracle's render path and to the second reading): nothing outside 1e-9 of the pixel's term scale, the
     albedo sums the composition's BYTES (sums of constants in sample order: a differing byte is a different first hit); at most 3 pixels a
     frame may leave through first_hit_ref.account_for_off_pixels (one fragile sample each, printed);
  b  the axis rule is the general test: a scene created under RMD_TUNE_AXIS_PAIRS = 1 gives the same F and G bit for bit, three_grids also under
     and without its mask budget;
  c  the contract's exact properties off the stock scene: sample ranges add up, rect lists on and off the 8-pixel lattice agree, uncovered pixels
     and a NULL second buffer keep their bytes, and under the lens the albedo sums are the render kernel's own first hits;
  d  lens edges: focal lengths -2.5 (no sample has a ray), 0, 1e-3, 1e6 and NaN, apertures 1e-9, 4 (wider than the room) and 0;
  e  the object table either side of the 64 KiB dynamic-LDS opt-in of launch_features and at the largest table check_render_args accepts, without
     and with a grid whose occupancy mask fills its budget; one object more is RMD_ERR_UNSUPPORTED from both forms, the buffers untouched.
"""
import ctypes as C
import json

import numpy as np
import pytest

import first_hit_ref as fr
import mesh_scenes as ms
import sphere_scenes as ss
from raymond_amd import abi, probe, render
from raymond_amd.scene import CameraSettings, Object, Plane, Scene, Settings, Sphere, Transform, generate_tiles, tile_array
from test_gpu_parity import same_bits
from test_gpu_sphere_scenes import rect_lists
from test_mesh_scenes_host import without_grids

pytestmark = pytest.mark.gpu

KEYS = fr.feature_keys()
EDGE_KEYS = fr.feature_keys(lens_edges=True)
NO_WALLS = ("open_scene", "mirror_box")  # and no_ray_enters 0, 1: the mesh classes without a plane
AXIS_KEYS = [k for k in KEYS if k[1] not in NO_WALLS and not (k[1] == "no_ray_enters" and k[2] < 2)]
EXACT_KEYS = ([("spheres", n, s, True, None) for n in ("camera_on_walls", "coincident_spheres") for s in (0, 1)] +
              [("mesh", n, s, True, None) for n in ("camera_in_box", "mirror_box") for s in (0, 1)] +
              [("spheres", "table_edges", s, False, None) for s in (4, 5, 6, 7)] + [("mesh", "grid_positions", s, False, None) for s in (2, 3, 4, 5)] +
              [("mesh", "nan_normals", s, False, None) for s in (0, 1)] + [("spheres", "fov_and_aspect", s, False, None) for s in (0, 1)])
PROBED_KEYS = (("spheres", "camera_on_walls", 0, True, None), ("mesh", "camera_in_box", 0, True, None))
MISSING_EDGE = fr.EDGE_EXTRA[0]  # the wide aperture over a scene without walls: here samples do miss
TUNABLES = (abi.RMD_TUNE_AXIS_PAIRS, abi.RMD_TUNE_MASK_BUDGET)


def ids(keys):
    return [fr.feature_key_id(k) for k in keys]


@pytest.fixture(scope="module")
def ctx(product_lib):
    """A context of this module's own: the tests change its tunables."""
    with render.Context(0) as c:
        yield c


class Device:
    """One feature case's scene on the device and its feature passes."""

    def __init__(self, ctx, fc):
        self.ctx, self.fc = ctx, fc
        self.W, self.H = fc.cam.backbuffer_width, fc.cam.backbuffer_height
        self.open, self.scenes = [], {}
        self.fb, self.fb_sq = render.FeatureBuffer(ctx, self.W, self.H), render.FeatureBuffer(ctx, self.W, self.H)
        self.open += [self.fb, self.fb_sq]
        self.tiles = generate_tiles(self.W, self.H, (32, 32))

    def scene(self, under=None):
        """the scene as created under the case's own tunables and `under` (read when the scene is created); one upload per setting"""
        under = {**self.fc.tunables, **(under or {})}
        key = tuple(sorted(under.items()))
        if key not in self.scenes:
            for k in TUNABLES:
                self.ctx.set_tunable(k, under.get(k, 0))
            try:
                self.scenes[key] = render.DeviceScene(self.ctx, self.fc.scene)
            finally:
                for k in TUNABLES:
                    self.ctx.set_tunable(k, 0)
            self.open.append(self.scenes[key])
        return self.scenes[key]

    def run(self, ds=None, rects=None, ranges=None, base=None, with_sq=True, settings=None):
        """-> (F, G) after the feature passes over `rects` (the frame in 32 x 32 tiles) and `ranges` (the case's samples) into buffers that start
        from `base` = (F0, G0) or zero"""
        st = settings or self.fc.settings
        if base is None:
            self.fb.zero(), self.fb_sq.zero()
        else:
            self.fb.upload(base[0]), self.fb_sq.upload(base[1])
        for begin, count in ranges or [(self.fc.begin, self.fc.spp)]:
            render.render_features(self.ctx, ds or self.scene(), st.camera_settings, st, self.tiles if rects is None else rects, self.fb, begin, count,
                                   features_sq=self.fb_sq if with_sq else None)
        return self.fb.download(), self.fb_sq.download()

    def run_sample(self, x, y, s):
        F, G = self.run(rects=[(x, y, 1, 1)], ranges=[(s, 1)])
        return F[y, x], G[y, x]

    def close(self):
        for k in TUNABLES:
            self.ctx.set_tunable(k, 0)
        for o in self.open:
            o.close()


def record(entry):
    """one line per frame held to the oracle: the figures profiles/r23_features_scenes/README.md is made of (pytest -s, or -rP, shows them)"""
    print("features scenes: %s" % json.dumps(entry))


def hold_to_the_oracle(dev, key, F, G, label=None):
    """the bars of a: nothing outside 1e-9 of the pixel's term scale, the albedo sums the composition's bytes; what is, accounted for"""
    ref = fr.reference(key)
    label = label or fr.feature_key_id(key)
    bad = fr.outside_the_pixel_bar(F, ref.F, ref.TF) | fr.outside_the_pixel_bar(G, ref.G, ref.TG)
    for d, r in ((F, ref.F), (G, ref.G)):
        bad[..., 3:6] |= np.ascontiguousarray(d[..., 3:6]).view(np.uint64) != np.ascontiguousarray(r[..., 3:6]).view(np.uint64)
    worst_f, worst_g = fr.worst_over_scale(F, ref.F, ref.TF), fr.worst_over_scale(G, ref.G, ref.TG)
    entry = {"case": label, "pixels": int(bad.shape[0] * bad.shape[1]), "worst_F_over_T": worst_f, "worst_G_over_T": worst_g,
             "values_outside": int(bad.sum()), "accounted_pixels": 0}
    try:
        if bad.any():
            entry["accounted_pixels"] = fr.account_for_off_pixels(dev.fc, (F, G), bad, dev.run_sample, label)
    finally:
        record(entry)
    return ref


# ---------------------------------------------------------------- a
@pytest.mark.parametrize("key", KEYS, ids=ids(KEYS))
def test_every_case_against_the_oracle(ctx, oracle, key):
    dev = Device(ctx, fr.feature_case(key))
    try:
        F, G = dev.run()
        hold_to_the_oracle(dev, key, F, G)
    finally:
        dev.close()


# ---------------------------------------------------------------- b
@pytest.mark.parametrize("key", AXIS_KEYS, ids=ids(AXIS_KEYS))
def test_the_axis_rule_is_the_general_test_bit_for_bit(ctx, key):
    fc = fr.feature_case(key)
    assert any(isinstance(o.geometry, Plane) for o in fc.scene.objects)
    dev = Device(ctx, fc)
    try:
        base = prefill(key, dev.W, dev.H)
        F, G = dev.run(base=base)
        general = dev.scene({abi.RMD_TUNE_AXIS_PAIRS: 1})
        fields = ss.expected_axis_pairs(without_grids(fc.scene))  # (the pairs are the planes' own, whatever the grids)
        assert probe.scene_plan(general)["axis_pairs"] == 0
        assert probe.scene_plan(dev.scene())["axis_pairs"] == fields[0] | fields[1] << 10 | fields[2] << 20
        settings = [{abi.RMD_TUNE_AXIS_PAIRS: 1}]
        if key[1] == "three_grids":  # under and without its mask budget, either rule
            other = 0 if fc.tunables else 256
            settings += [{abi.RMD_TUNE_MASK_BUDGET: other}, {abi.RMD_TUNE_MASK_BUDGET: other, abi.RMD_TUNE_AXIS_PAIRS: 1}]
        for under in settings:
            F2, G2 = dev.run(ds=dev.scene(under), base=base)
            assert same_bits(F2, F).all() and same_bits(G2, G).all(), "%s: the scene created under %s gives other features" % (fr.feature_key_id(key), under)
        assert (F != base[0]).any() and (G != base[1]).any()
    finally:
        dev.close()


# ---------------------------------------------------------------- c
def prefill(key, W, H):
    rng = np.random.default_rng([key[2], int(key[3]), len(key[1])])
    return rng.uniform(0.25, 3.0, (H, W, 7)), rng.uniform(0.25, 3.0, (H, W, 7))


@pytest.mark.parametrize("key", EXACT_KEYS, ids=ids(EXACT_KEYS))
def test_the_contracts_exact_properties_off_the_stock_scene(ctx, key):
    fc = fr.feature_case(key)
    dev = Device(ctx, fc)
    try:
        W, H, b, n = dev.W, dev.H, fc.begin, fc.spp
        base = prefill(key, W, H)
        full = [(0, 0, W, H)]
        one = dev.run(rects=full, base=base)
        assert (one[0] != base[0]).any() and (one[1] != base[1]).any()
        same = lambda a, r: bool(same_bits(a, r).all())  # (NaN for NaN: nan_normals)
        # [0, 2) + [2, 6) == [0, 6)
        two = dev.run(rects=full, ranges=[(b, 2), (b + 2, n - 2)], base=base)
        assert same(two[0], one[0]) and same(two[1], one[1])
        # one rect == 8 x 8 tiles == 5 x 3 tiles
        for ts in ((8, 8), (5, 3)):
            cut = dev.run(rects=generate_tiles(W, H, ts), base=base)
            assert same(cut[0], one[0]) and same(cut[1], one[1]), ts
        # the two rect lists off the 8-pixel lattice: covered pixels agree, the others keep the pre-fill's bytes
        for rects in rect_lists(W, H):
            covered = np.zeros((H, W), dtype=bool)
            for (l, t, w, h) in rects:
                assert w > 0 and h > 0 and l + w <= W and t + h <= H and not covered[t : t + h, l : l + w].any()
                covered[t : t + h, l : l + w] = True
            assert covered.any() and not covered.all()
            got = dev.run(rects=rects, base=base)
            for j in (0, 1):
                assert same(got[j][covered], one[j][covered]), rects[:2]
                assert got[j][~covered].tobytes() == base[j][~covered].tobytes(), rects[:2]
        # feat_sq = NULL: F the same bits, the second buffer's bytes left
        nosq = dev.run(rects=full, base=base, with_sq=False)
        assert same(nosq[0], one[0]) and nosq[1].tobytes() == base[1].tobytes()
        if key in PROBED_KEYS:  # the albedo sums are the render kernel's own first hits under the lens
            assert fc.use_dof and fc.cam.aperture_radius > 0.0
            xy, _ = fr.pixel_grid(W, H)
            colors = np.array([list(o.material.color) for o in fc.scene.objects] + [[0.0, 0.0, 0.0]])  # index -1: a miss / no ray
            A, A2 = base[0][..., 3:6].reshape(-1, 3), base[1][..., 3:6].reshape(-1, 3)
            for s in range(b, b + n):
                _, po, _ = probe.trace_samples(ctx, dev.scene(), fc.cam, fc.settings, xy, np.full(len(xy), s, dtype=np.uint32), paths=True)
                first = np.where(po[:, 0] >= 0, po[:, 0], -1)
                A, A2 = A + colors[first], A2 + colors[first] * colors[first]
            assert one[0][..., 3:6].tobytes() == A.reshape(H, W, 3).tobytes() and one[1][..., 3:6].tobytes() == A2.reshape(H, W, 3).tobytes()
            st0 = Settings(CameraSettings(W, H, fc.cam.fov_vert, fc.cam.transform, focal_length=fc.cam.focal_length), sample_count=n, bounce_limit=1, seed=fc.seed)
            assert dev.run(rects=full, base=base, settings=st0)[0].tobytes() != one[0].tobytes()  # the lens moved some first hits
    finally:
        dev.close()


# ---------------------------------------------------------------- d
@pytest.mark.parametrize("key", EDGE_KEYS, ids=ids(EDGE_KEYS))
def test_lens_edges_against_the_oracle(ctx, oracle, key):
    fc = fr.feature_case(key)
    edge = key[4]
    dev = Device(ctx, fc)
    try:
        F, G = dev.run()
        ref = hold_to_the_oracle(dev, key, F, G)
        W, H = dev.W, dev.H
        xy, pix = fr.pixel_grid(W, H)
        rays, ok = oracle.sample_primary_rays(fc.cam, fc.seed, True, xy, np.full(len(pix), fc.begin, dtype=np.uint32))
        base = prefill(key, W, H)
        if edge in ("focal-negative", "focal-nan"):  # no sample has a ray: the oracle's ok is 0 everywhere, and a strictly positive pre-fill keeps its bytes
            assert not ok.any() and (ref.objs == -1).all() and not ref.F.any() and not ref.G.any()
            kept = dev.run(base=base)
            assert kept[0].tobytes() == base[0].tobytes() and kept[1].tobytes() == base[1].tobytes()
        else:
            assert ok.all() and (ref.objs >= 0).any()
        if edge == "focal-zero":  # the rays lie in the lens plane: rd.z == 0 exactly, and the z pair faces neither wall
            assert (rays[:, 5] == 0.0).all()
            z_walls = [i for i, o in enumerate(fc.scene.objects) if isinstance(o.geometry, Plane) and o.geometry.normal[2] != 0.0]
            assert len(z_walls) == 2 and not np.isin(ref.objs, z_walls).any()
        if edge == "aperture-zero":  # use_dof with a closed aperture: the pinhole call's bytes
            st0 = Settings(fc.cam, sample_count=fc.spp, bounce_limit=1, seed=fc.seed, use_dof=False)
            F0, G0 = dev.run(settings=st0)
            assert F0.tobytes() == F.tobytes() and G0.tobytes() == G.tobytes()
        if edge == "aperture-4":  # wider than the room: origins outside the walls, one-sided planes passed from behind
            walls = [o.geometry for o in fc.scene.objects if isinstance(o.geometry, Plane) and abs(o.geometry.normal[0]) == 1.0 and o.geometry.normal[1] == 0.0]
            if key != MISSING_EDGE:
                assert len(walls) == 2
                lo, hi = sorted(w.origin[0] for w in walls)
                assert ((rays[:, 0] < lo) | (rays[:, 0] > hi)).any()
                # every primary ray runs towards +z and the far wall is an unbounded plane that faces it: in a closed room none misses
                assert (ref.objs >= 0).all()
            else:
                assert (ref.objs < 0).any() and (ref.objs >= 0).any()
    finally:
        dev.close()


# ---------------------------------------------------------------- e
def table_scene(n_total, grid=None):
    """six walls, the grid object if any, and small spheres up to n_total objects; the spheres FIRST (the walls end the table)"""
    rng = np.random.default_rng([0x7AB1E, n_total])
    lo, hi = [-2.0, -1.5, -1.0], [2.0, 1.5, 3.5]
    walls = [w[0] for w in ss._room(rng, lo, hi)]
    n = n_total - 6 - (1 if grid is not None else 0)
    sc = Scene()
    for _ in range(n):
        c = (rng.uniform(-1.6, 1.6), rng.uniform(-1.2, 1.2), rng.uniform(1.0, 3.0))
        sc.objects.append(Object(Sphere(c, float(rng.uniform(0.01, 0.04))), ss._material(rng)))
    if grid is not None:
        sc.objects.insert(n // 2, Object(grid, ss._diffuse(rng)))
    sc.objects += walls
    assert len(sc.objects) == n_total
    return sc


def check_table(ctx, sc, label, accepted):
    W, H, spp, seed = 16, 16, 4, 0x7AB1E
    cam = CameraSettings(W, H, 55.0, Transform((0.0, 0.0, 0.0)))
    fc = fr.FeatureCase(None, sc, cam, Settings(cam, sample_count=spp, bounce_limit=1, seed=seed), seed, False, 0, spp, {})
    dev = Device(ctx, fc)
    try:
        ds = dev.scene()
        n, g, m = probe.scene_layout(ds)
        if accepted:
            F, G = dev.run()
            F_ref, G_ref, objs, TF, TG, _ = fr.first_hit_sums(sc, cam, seed, spp, scales=True)
            bad = fr.outside_the_pixel_bar(F, F_ref, TF) | fr.outside_the_pixel_bar(G, G_ref, TG)
            for d, r in ((F, F_ref), (G, G_ref)):
                bad[..., 3:6] |= np.ascontiguousarray(d[..., 3:6]).view(np.uint64) != np.ascontiguousarray(r[..., 3:6]).view(np.uint64)
            entry = {"case": label, "pixels": W * H, "worst_F_over_T": fr.worst_over_scale(F, F_ref, TF), "worst_G_over_T": fr.worst_over_scale(G, G_ref, TG),
                     "values_outside": int(bad.sum()), "accounted_pixels": 0, "objects": n, "mask_words": m, "distinct_first_hits": int(len(np.unique(objs)))}
            try:
                if bad.any():
                    entry["accounted_pixels"] = fr.account_for_off_pixels(fc, (F, G), bad, dev.run_sample, label)
            finally:
                record(entry)
            assert len(np.unique(objs)) > 10  # the table's spheres are seen
            return n, g, m
        base = prefill(("", "", n, False, None), W, H)
        dev.fb.upload(base[0]), dev.fb_sq.upload(base[1])
        c, s, rects = cam.pod(), fc.settings.pod(0, spp), tile_array([(0, 0, W, H)])
        for fn in (ctx.L.rmd_render_features, ctx.L.rmd_render_features_async):
            assert fn(ctx.handle, ds.handle, C.byref(c), C.byref(s), rects, 1, dev.fb.ptr, dev.fb_sq.ptr) == abi.RMD_ERR_UNSUPPORTED, label
        ctx.synchronize()
        assert dev.fb.download().tobytes() == base[0].tobytes() and dev.fb_sq.download().tobytes() == base[1].tobytes()
        return n, g, m
    finally:
        dev.close()


def test_the_object_table_at_the_lds_edges(ctx, oracle):
    tiles, buffered = probe.launch_sizes(probe.MODE_TILES, False), probe.launch_sizes(probe.MODE_TILES_BUFFERED, False)
    optin = 64 * 1024
    lds = lambda n: int(probe.launch_plan(probe.MODE_TILES, False, [n], [0], 0, 4, 0)["lds"][0])  # launch_features' plan: one wave per item
    below = (optin - tiles["wave"]) // tiles["object"]
    assert lds(below) <= optin < lds(below + 1)
    largest = (tiles["budget"] - buffered["wave"]) // tiles["object"]  # check_render_args: the table beside one wave's area and the sort pool
    assert below + 1 < largest and lds(largest) <= tiles["budget"]
    for n, label, accepted in ((below, "at the opt-in", True), (below + 1, "past the opt-in", True), (largest, "largest table", True), (largest + 1, "one more", False)):
        got = check_table(ctx, table_scene(n), "object table %s: %d objects" % (label, n), accepted)
        assert got[:2] == (n, 0)


def test_the_object_table_at_the_lds_edge_with_a_full_mask(ctx, oracle):
    """mesh_scenes' lumpy mesh at n = 106 builds in under a second to 392,000 cells: 12,251 mask words of the budget's 12,288"""
    sizes = probe.launch_sizes(probe.MODE_TILES, True)
    grid = ms._grid(ms._lumpy(106, (1.5, 1.25, 0.75), (0.0, 0.0, 2.0)))
    _, g, m = check_table(ctx, table_scene(64, grid), "full mask: 64 objects", True)
    assert g == 1 and 0.97 * sizes["mask_budget"] <= 4 * m <= sizes["mask_budget"], m
    largest = (sizes["budget"] - 4 * ((m + 3) // 4 * 4) - sizes["wave"]) // sizes["object"]  # check_render_args: table + masks + one wave's area
    assert largest > 700
    assert check_table(ctx, table_scene(largest, grid), "full mask, largest table: %d objects" % largest, True) == (largest, 1, m)
    assert check_table(ctx, table_scene(largest + 1, grid), "full mask, one more: %d objects" % (largest + 1), False) == (largest + 1, 1, m)
