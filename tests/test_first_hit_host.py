"""The first-hit composition of tests/first_hit_ref.py on the CPU, before the device is held to it (tests/test_gpu_features_scenes.py).

  * orc_sample_primary_rays with use_dof = False gives, byte for byte, the rays of the former composition (orc_block_uniforms -> orc_primary_ray);
  * on every case of sphere_scenes.cases() and mesh_scenes.cases(), the thin-lens variants included, and on the lens-edge cameras (negative, zero,
    tiny, huge and NaN focal lengths; apertures of 1e-9, 4 and 0): orc_scene_intersect on those rays gives the first vertex of orc_trace_sample —
    the composition IS the render path's first hit — and where the entry reports no ray the oracle's sample is (0, 0, 0) with an empty path;
  * on the same (pixel, sample) pairs the second reading of the source (tests/second_reading.py) gives the same ray, object, triangle, t and
    normal, bit for bit (NaN for NaN), and raises Panic exactly where ok == 0;
  * the classes are what the feature tests need them to be: which miss, which hold triangle hits, hits at t == 0, NaN normals, the table's reach.
"""
import numpy as np
import pytest

import first_hit_ref as fr
import second_reading as sr
from test_second_reading import same_f64, second_reading_scene

KEYS = fr.feature_keys()
EDGE_KEYS = fr.feature_keys(lens_edges=True)
N_PAIRS = 200


def pairs_of(key, fc):
    """a seeded list of N_PAIRS (x, y, sample) triples of the case's frame and sample range"""
    rng = np.random.default_rng([0xF157, key[2], int(key[3])] + [ord(c) for c in key[1] + (key[4] or "")])
    W, H = fc.cam.backbuffer_width, fc.cam.backbuffer_height
    xy = np.stack([rng.integers(0, W, N_PAIRS), rng.integers(0, H, N_PAIRS)], axis=1).astype(np.uint32)
    return xy, rng.integers(fc.begin, fc.begin + fc.spp, N_PAIRS).astype(np.uint32)


def test_the_pinhole_rays_are_the_former_compositions_bytes(oracle):
    from raymond_amd.scene import CameraSettings, Transform

    for (W, H), fov, pos, seed in (((40, 24), 55.0, (0.0, 0.0, 0.0), 0x5CE7E000), ((97, 9), 5.1, (0.125, -0.125, 0.0), 7), ((9, 97), 149.0, (-2.5, 0.0, 0.5), 2**40 + 3),
                                   ((16, 16), 55.0, (0.0, 0.0, 0.0), 11), ((44, 27), 55.0, (0.0, 0.0, 0.0), 0x3E5E000)):
        xy, pix = fr.pixel_grid(W, H)
        for aperture in (0.0, 0.5):
            cam = CameraSettings(W, H, fov, Transform(pos), focal_length=2.5, aperture_radius=aperture)
            for s in (0, 5, 2**31 + 1):
                rays, ok = oracle.sample_primary_rays(cam, seed, False, xy, np.full(len(pix), s, dtype=np.uint32))
                assert ok.all() and rays.tobytes() == fr.pinhole_rays(cam, seed, xy, pix, s).tobytes()
        # use_dof with a closed aperture is the pinhole ray too (what RMD_RENDER_DOF selects)
        cam = CameraSettings(W, H, fov, Transform(pos), focal_length=2.5, aperture_radius=0.0)
        rays, ok = oracle.sample_primary_rays(cam, seed, True, xy, np.full(len(pix), 3, dtype=np.uint32))
        assert ok.all() and rays.tobytes() == fr.pinhole_rays(cam, seed, xy, pix, 3).tobytes()


@pytest.mark.parametrize("key", KEYS + EDGE_KEYS, ids=[fr.feature_key_id(k) for k in KEYS + EDGE_KEYS])
def test_the_composition_is_the_render_paths_first_hit_and_the_second_readings(oracle, key):
    fc = fr.feature_case(key)
    osc = oracle.OracleScene(fc.scene)
    xy, smp = pairs_of(key, fc)
    phi, obj, t, sub, ok, rays = fr.sample_features(fc.scene, osc, fc.cam, fc.seed, fc.use_dof, xy, smp)
    sc, c = second_reading_scene(fc.scene, fc.cam)
    lens = fc.use_dof and fc.cam.aperture_radius > 0.0  # what RMD_RENDER_DOF selects: the lens only with an open aperture
    W = fc.cam.backbuffer_width
    for i in range(N_PAIRS):
        x, y, s = int(xy[i, 0]), int(xy[i, 1]), int(smp[i])
        # the render path
        rgb, po, ps = osc.trace_sample_path(fc.cam, fc.settings, x, y, s)
        if not ok[i]:
            assert len(po) == 0 and not rgb.any() and obj[i] == -1 and not phi[i].any(), (x, y, s)
        else:
            assert len(po) == 1 and po[0] == obj[i] and (obj[i] < 0 or ps[0] == sub[i]), (x, y, s, po, ps, obj[i], sub[i])
        # the second reading
        stream = sr.Stream(fc.seed, y * W + x, s)
        try:
            o2, d2 = (sr.generate_primary_ray_with_dof if lens else sr.generate_primary_ray)(x, y, c, stream)
        except sr.Panic:
            assert not ok[i], (x, y, s)
            continue
        assert ok[i], (x, y, s)
        assert all(same_f64(a, b) for a, b in zip(tuple(o2) + tuple(d2), rays[i])), (x, y, s, o2, d2, rays[i])
        found = sr.scene_intersect(sc["objects"], o2, d2)
        if found is None:
            assert obj[i] == -1 and not phi[i].any(), (x, y, s)
            continue
        oi, dist, tri = found
        assert (oi, tri) == (int(obj[i]), int(sub[i])) and same_f64(dist, t[i]), (x, y, s, found, obj[i], t[i], sub[i])
        o = sc["objects"][oi]
        if o["kind"] == "plane":
            normal = o["normal"]
        elif o["kind"] == "sphere":
            normal = sr.normalize(sr.sub(sr.add(o2, sr.scale(d2, dist)), o["origin"]))
        else:
            p, n = o["grid"]["tri_pos"][tri], o["grid"]["tri_nrm"][tri]
            normal = sr.triangle_normal((p[0:3], p[3:6], p[6:9]), (n[0:3], n[3:6], n[6:9]), o2, d2, dist)
        assert all(same_f64(a, b) for a, b in zip(normal, phi[i, 0:3])), (x, y, s, normal, phi[i])
        assert tuple(phi[i, 3:6]) == tuple(o["material"][1]) and same_f64(phi[i, 6], dist)
    if key[4] == "focal-negative" or key[4] == "focal-nan":
        assert not ok.any()
    elif key[4] is not None or not lens:
        assert ok.all()  # (a pinhole sample always has a ray; so has a lens sample with the focal plane ahead of the camera)


@pytest.mark.parametrize("key", KEYS, ids=[fr.feature_key_id(k) for k in KEYS])
def test_the_classes_are_what_the_feature_tests_need(oracle, key):
    kind, name, seed, lens, _ = key
    fc, ref = fr.feature_case(key), fr.reference(key)
    flat = fc.scene.flatten()[0]
    hit_kinds = {int(flat[i].geometry_kind) for i in np.unique(ref.objs) if i >= 0}
    missed = float((ref.objs < 0).mean())
    at_zero = int((ref.t == 0.0).sum())
    n_nan = int(np.isnan(ref.F).sum())
    print("%s: %.3f of samples miss, hit kinds %s, %d distinct first-hit objects, %d hits at t == 0, %d NaN values in F" % (
        fr.feature_key_id(key), missed, sorted(hit_kinds), len(np.unique(ref.objs[ref.objs >= 0])), at_zero, n_nan))
    assert (np.nan_to_num(ref.F, nan=1.0) != 0.0).any()
    assert ref.F.shape == (fc.cam.backbuffer_height, fc.cam.backbuffer_width, 7) and ref.objs.shape[0] == fr.FEATURE_SPP
    if kind == "spheres":
        assert missed == 0.0  # partial_room too: its open directions are not in view
    if name == "open_scene" or (name == "no_ray_enters" and seed < 2):  # 0.75 to 0.87, to two places, of samples 0 .. 5 (measured from sample 0)
        missed0 = float((fr.first_hit_sums(fc.scene, fc.cam, fc.seed, fr.FEATURE_SPP, 0, use_dof=fc.use_dof)[2] < 0).mean())
        assert 0.75 <= round(missed0, 2) <= 0.87 and 0.70 <= missed <= 0.90, (missed0, missed)
    if kind == "mesh":
        assert (2 in hit_kinds) == (name != "no_ray_enters")
    if (name == "camera_on_walls" and not lens and seed in (0, 1, 5, 6, 7)) or name == "camera_on_wall_with_mesh":
        assert at_zero > 0
    if (name, seed, lens) == ("camera_on_walls", 2, False):  # one step inside the wall: the facing rays meet it a few ulps away
        assert 0.0 < np.nanmin(np.where(ref.t > 0.0, ref.t, np.nan)) < 1e-14
    if name == "nan_normals":
        assert (n_nan > 0) == (seed == 1)
        if seed == 1:  # 180 values over samples 0 .. 5
            assert int(np.isnan(fr.first_hit_sums(fc.scene, fc.cam, fc.seed, fr.FEATURE_SPP, 0)[0]).sum()) == 180
    if name == "table_edges" and seed >= 4:
        assert len(np.unique(ref.objs)) > 300
    if name == "coincident_spheres":  # the twins are the first two Sphere objects of radius 0.375 at one centre: the lower index is seen, the higher never
        twins = [i for i, o in enumerate(fc.scene.objects) if getattr(o.geometry, "radius", None) == 0.375]
        assert len(twins) == 2 and fc.scene.objects[twins[0]].geometry.origin == fc.scene.objects[twins[1]].geometry.origin
        assert (ref.objs == twins[0]).any() and not (ref.objs == twins[1]).any()


def test_a_fragile_hit_is_told_from_a_sound_one(oracle):
    """the accounting's own judge, on hits whose kind is known: a twin sphere's hit is tied, a wall seen head-on is neither tied nor grazing"""
    key = ("spheres", "coincident_spheres", 0, False, None)
    fc, ref = fr.feature_case(key), fr.reference(key)
    osc = oracle.OracleScene(fc.scene)
    twins = [i for i, o in enumerate(fc.scene.objects) if getattr(o.geometry, "radius", None) == 0.375]
    walls = [i for i, o in enumerate(fc.scene.objects) if hasattr(o.geometry, "normal")]
    W = fc.cam.backbuffer_width
    xy, pix = fr.pixel_grid(W, fc.cam.backbuffer_height)
    phi, obj, t, sub, ok, rays = fr.sample_features(fc.scene, osc, fc.cam, fc.seed, fc.use_dof, xy, np.full(len(pix), fc.begin, dtype=np.uint32))
    i = int(np.flatnonzero(obj == twins[0])[0])
    assert fr.fragile_hit(fc.scene, osc, rays[i], obj[i], t[i], sub[i]) == "tied"
    sound = [fr.fragile_hit(fc.scene, osc, rays[j], obj[j], t[j], sub[j]) for j in np.flatnonzero(np.isin(obj, walls))[:40]]
    assert sound.count(None) >= 30, sound  # (a wall hit beside a sphere's rim or a room's edge may be grazing; most are not)
    # and the accounting: a device that IS the composition has nothing to account for; one that differs on a sound hit fails
    dev = (ref.F.copy(), ref.G.copy())
    assert fr.account_for_off_pixels(fc, dev, np.zeros(ref.F.shape, dtype=bool), None, "self") == 0
    j = int(np.flatnonzero(np.isin(obj, walls))[sound.index(None)])
    x, y = int(xy[j, 0]), int(xy[j, 1])

    def run_sample(px, py, s, wrong=fc.begin):
        f = fr.sample_features(fc.scene, osc, fc.cam, fc.seed, fc.use_dof, [[px, py]], [s])[0][0].copy()
        if s == wrong:
            f[6] *= 1.0 + 1e-6
        return f, f * f

    dev[0][y, x], dev[1][y, x] = np.zeros(7), np.zeros(7)
    for s in range(fc.begin, fc.begin + fc.spp):
        f, g = run_sample(x, y, s)
        dev[0][y, x], dev[1][y, x] = dev[0][y, x] + f, dev[1][y, x] + g
    bad = fr.outside_the_pixel_bar(dev[0], ref.F, ref.TF)
    assert bad[y, x, 6] and bad.sum() == 1
    with pytest.raises(AssertionError, match="neither grazing nor tied"):
        fr.account_for_off_pixels(fc, dev, bad, run_sample, "wrong depth")
