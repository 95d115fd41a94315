"""rmd_render_features on the device: the sums against the oracle's composition (tests/first_hit_ref.py), the render kernel's own first hits
under the thin lens, the exact properties of the contract, the refused arguments, and that the pass leaves a context's renders alone."""
import ctypes as C

import numpy as np
import pytest

import first_hit_ref
from raymond_amd import abi, probe, render, scenes
from raymond_amd.scene import Material, Object, Plane, Scene, Settings, Sphere, generate_tiles, tile_array

pytestmark = pytest.mark.gpu

INFO_FIELDS = ("passes", "split_k", "persistent", "end_black_paths", "has_grid", "waves_per_workgroup", "buffered", "chained", "queued")


def info_tuple(ctx):
    i = ctx.last_launch_info()
    return tuple(getattr(i, f) for f in INFO_FIELDS)


def features(ctx, ds, st, tiles, begin=0, count=None, with_sq=True, base=None):
    """(F, G) of rmd_render_features over `tiles` into buffers that start from `base` = (F0, G0) or zero."""
    cam = st.camera_settings
    W, H = cam.backbuffer_width, cam.backbuffer_height
    fb, fb_sq = render.FeatureBuffer(ctx, W, H), render.FeatureBuffer(ctx, W, H)
    try:
        if base is not None:
            fb.upload(base[0]), fb_sq.upload(base[1])
        render.render_features(ctx, ds, cam, st, tiles, fb, begin, count, features_sq=fb_sq if with_sq else None)
        return fb.download(), fb_sq.download()
    finally:
        fb.close(), fb_sq.close()


def open_scene():
    """One sphere, one tilted floor plane, no room: most primary rays miss."""
    sc = Scene()
    sc.objects.append(Object(Sphere((0.3, 0.2, 3.0), 0.6), Material.Metal((0.9, 0.6, 0.2), 0.2)))
    sc.objects.append(Object(Plane((0.0, -1.5, 0.0), (0.0, 1.0, 0.3)), Material.Diffuse((0.2, 0.7, 0.3), 0.5)))
    return sc


def check_against_the_oracle(ctx, sc, W, H, spp, seed=scenes.SEED):
    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=seed)
    F_ref, G_ref, objs = first_hit_ref.first_hit_sums(sc, st.camera_settings, seed, spp)
    ds = render.DeviceScene(ctx, sc)
    try:
        F, G = features(ctx, ds, st, generate_tiles(W, H, (32, 32)))
    finally:
        ds.close()
    for name, dev, ref in (("F", F, F_ref), ("G", G, G_ref)):
        bad = first_hit_ref.outside_the_bar(dev, ref)
        with np.errstate(all="ignore"):
            worst = np.nanmax(np.abs(dev - ref))
        print("features %s: %d of %d values outside 1e-9 of the group scale, largest |dev - ref| %.3g" % (name, bad.sum(), bad.size, worst))
        assert not bad.any(), "%s: %d values outside the bar, first at %s" % (name, bad.sum(), np.argwhere(bad)[0])
    return F, G, objs


@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_features_match_the_oracle_composition(gpu_ctx, oracle, which):
    sc = scenes.reflective_spheres() if which == "spheres" else scenes.gold_dragon_standin(n=24)
    F, G, objs = check_against_the_oracle(gpu_ctx, sc, 256, 144, 8)
    assert (objs >= 0).all()  # closed rooms: no miss
    kinds = {int(sc.flatten()[0][i].geometry_kind) for i in np.unique(objs)}
    assert kinds == ({0, 1} if which == "spheres" else {0, 1, 2})  # plane, sphere (and triangle) first hits all occur
    assert np.isfinite(F).all() and np.isfinite(G).all() and (F[..., 6] > 0).all()


def test_open_scene_misses_are_zeros(gpu_ctx, oracle):
    sc = open_scene()
    F, G, objs = check_against_the_oracle(gpu_ctx, sc, 96, 54, 4)
    miss_all = (objs < 0).all(axis=0)
    assert miss_all.mean() > 0.5 and (objs == 0).any() and (objs == 1).any()
    assert not F[miss_all].any() and not G[miss_all].any()  # exactly zero, both signs of zero aside
    assert F[~miss_all].any()


@pytest.mark.parametrize("use_dof", [False, True])
def test_albedo_sums_equal_the_render_kernels_own_first_hits(gpu_ctx, use_dof):
    """path_obj[0] / path_sub[0] of rmd_probe_trace_samples are the render kernel's first hits (the thin lens included): the albedo sums are sums
    of constants and must match bit for bit."""
    W, H, spp = 64, 40, 4
    sc = scenes.reflective_spheres()
    st = Settings(scenes.camera(W, H, aperture_radius=0.08 if use_dof else 0.0), sample_count=spp, bounce_limit=3, seed=scenes.SEED, use_dof=use_dof)
    ds = render.DeviceScene(gpu_ctx, sc)
    try:
        F, G = features(gpu_ctx, ds, st, generate_tiles(W, H, (32, 32)))
        xy, _ = first_hit_ref.pixel_grid(W, H)
        colors = np.array([list(o.material.color) for o in sc.objects] + [[0.0, 0.0, 0.0]])  # index -1: a miss / no ray
        A, A2 = np.zeros((H * W, 3)), np.zeros((H * W, 3))
        firsts = []
        for s in range(spp):
            _, po, _ = probe.trace_samples(gpu_ctx, ds, st.camera_settings, st, xy, np.full(len(xy), s, dtype=np.uint32), paths=True)
            first = np.where(po[:, 0] >= 0, po[:, 0], -1)
            firsts.append(first)
            A = A + colors[first]
            A2 = A2 + colors[first] * colors[first]
        assert F[..., 3:6].tobytes() == A.reshape(H, W, 3).tobytes()
        assert G[..., 3:6].tobytes() == A2.reshape(H, W, 3).tobytes()
        if use_dof:  # the lens moved some first hits: the pair differs
            st0 = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=3, seed=scenes.SEED)
            F0, _ = features(gpu_ctx, ds, st0, generate_tiles(W, H, (32, 32)))
            assert F0.tobytes() != F.tobytes()
    finally:
        ds.close()


@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_exact_properties_of_the_contract(gpu_ctx, which):
    W, H, n, k = 45, 29, 7, 3  # not multiples of 8: ragged wave tiles
    sc = scenes.reflective_spheres() if which == "spheres" else scenes.gold_dragon_standin(n=12)
    st = Settings(scenes.camera(W, H), sample_count=n, bounce_limit=5, seed=scenes.SEED + 3)
    rng = np.random.default_rng(1)
    base = rng.uniform(0, 1, (H, W, 7)), rng.uniform(0, 1, (H, W, 7))
    full = [(0, 0, W, H)]
    ds = render.DeviceScene(gpu_ctx, sc)
    fb, fb_sq = render.FeatureBuffer(gpu_ctx, W, H), render.FeatureBuffer(gpu_ctx, W, H)
    try:
        one = features(gpu_ctx, ds, st, full, 0, n, base=base)
        assert (one[0] != base[0]).any() and (one[1] != base[1]).any()
        # [0, k) + [k, n) == [0, n)
        fb.upload(base[0]), fb_sq.upload(base[1])
        render.render_features(gpu_ctx, ds, st.camera_settings, st, full, fb, 0, k, features_sq=fb_sq)
        render.render_features(gpu_ctx, ds, st.camera_settings, st, full, fb, k, n - k, features_sq=fb_sq)
        assert fb.download().tobytes() == one[0].tobytes() and fb_sq.download().tobytes() == one[1].tobytes()
        # one rect == 32 x 32 tiles == 8 x 8 tiles == 5 x 3 tiles
        for ts in ((32, 32), (8, 8), (5, 3)):
            cut = features(gpu_ctx, ds, st, generate_tiles(W, H, ts), 0, n, base=base)
            assert cut[0].tobytes() == one[0].tobytes() and cut[1].tobytes() == one[1].tobytes(), ts
        # feat_sq_dev = NULL: F the same bits, the second buffer untouched
        nosq = features(gpu_ctx, ds, st, full, 0, n, with_sq=False, base=base)
        assert nosq[0].tobytes() == one[0].tobytes() and nosq[1].tobytes() == base[1].tobytes()
        # pixels outside the call's tiles are untouched
        part = [(8, 8, 16, 11), (30, 0, 15, 5)]
        got = features(gpu_ctx, ds, st, part, 0, n, base=base)
        mask = np.zeros((H, W), dtype=bool)
        for l, t, w, h in part:
            mask[t : t + h, l : l + w] = True
        for j in (0, 1):
            assert got[j][mask].tobytes() == one[j][mask].tobytes() and got[j][~mask].tobytes() == base[j][~mask].tobytes()
        # the async form, then a synchronise
        fb.upload(base[0]), fb_sq.upload(base[1])
        render.render_features(gpu_ctx, ds, st.camera_settings, st, full, fb, 0, n, sync=False, features_sq=fb_sq)
        gpu_ctx.synchronize()
        assert fb.download().tobytes() == one[0].tobytes() and fb_sq.download().tobytes() == one[1].tobytes()
        # bounce_limit and the black-path flag are ignored
        st2 = Settings(scenes.camera(W, H), sample_count=n, bounce_limit=0, seed=scenes.SEED + 3, end_black_paths=True)
        other = features(gpu_ctx, ds, st2, full, 0, n, base=base)
        assert other[0].tobytes() == one[0].tobytes() and other[1].tobytes() == one[1].tobytes()
    finally:
        fb.close(), fb_sq.close(), ds.close()


def test_refused_arguments_leave_the_buffers_alone(gpu_ctx):
    W, H = 24, 16
    st = Settings(scenes.camera(W, H), sample_count=2, seed=scenes.SEED)
    ds = render.DeviceScene(gpu_ctx, scenes.reflective_spheres())
    fb, fb_sq = render.FeatureBuffer(gpu_ctx, W, H), render.FeatureBuffer(gpu_ctx, W, H)
    L, h = gpu_ctx.L, gpu_ctx.handle
    base = np.random.default_rng(2).uniform(0, 1, (H, W, 7))
    try:
        fb.upload(base), fb_sq.upload(base)
        cam, pod = st.camera_settings.pod(), st.pod(0, 2)
        both = st.pod(0, 2)
        both.flags = abi.RMD_RENDER_TRACE_BLACK_PATHS | abi.RMD_RENDER_END_BLACK_PATHS
        over = st.pod(0xFFFFFFFF, 2)
        full = tile_array([(0, 0, W, H)])
        cases = [
            (ds.handle, cam, pod, full, 1, None, fb_sq.ptr),
            (ds.handle, cam, pod, full, 1, fb.ptr, fb.ptr),
            (ds.handle, cam, pod, None, 1, fb.ptr, fb_sq.ptr),
            (None, cam, pod, full, 1, fb.ptr, fb_sq.ptr),
            (ds.handle, cam, pod, tile_array([(0, 0, W + 1, H)]), 1, fb.ptr, fb_sq.ptr),
            (ds.handle, cam, pod, tile_array([(0, 0, 16, 16), (15, 0, 9, 16)]), 2, fb.ptr, fb_sq.ptr),
            (ds.handle, cam, both, full, 1, fb.ptr, fb_sq.ptr),
            (ds.handle, cam, over, full, 1, fb.ptr, fb_sq.ptr),
        ]
        for fn in (L.rmd_render_features, L.rmd_render_features_async):
            for sc, c, s, rects, n, F, G in cases:
                assert fn(h, sc, C.byref(c), C.byref(s), rects, n, F, G) == abi.RMD_ERR_INVALID_ARGUMENT
        gpu_ctx.synchronize()
        assert fb.download().tobytes() == base.tobytes() and fb_sq.download().tobytes() == base.tobytes()
        # no samples, no tiles: good calls that change nothing
        render.render_features(gpu_ctx, ds, st.camera_settings, st, [(0, 0, W, H)], fb, 0, 0, features_sq=fb_sq)
        render.render_features(gpu_ctx, ds, st.camera_settings, st, [], fb, 0, 2, features_sq=fb_sq)
        assert fb.download().tobytes() == base.tobytes() and fb_sq.download().tobytes() == base.tobytes()
    finally:
        fb.close(), fb_sq.close(), ds.close()


@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_a_feature_pass_between_two_renders_disturbs_nothing(gpu_ctx, which):
    W, H = 40, 24
    sc = scenes.reflective_spheres() if which == "spheres" else scenes.gold_dragon_standin(n=12)
    st = Settings(scenes.camera(W, H), sample_count=8, bounce_limit=4, seed=scenes.SEED)
    tiles = generate_tiles(W, H, (32, 32))
    ds = render.DeviceScene(gpu_ctx, sc)
    fb, fb_sq, ft = render.Framebuffer(gpu_ctx, W, H), render.Framebuffer(gpu_ctx, W, H), render.FeatureBuffer(gpu_ctx, W, H)
    try:
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb, 0, 4, framebuffer_sq=fb_sq)
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb, 4, 4, framebuffer_sq=fb_sq)
        plain, plain_info = (fb.download(), fb_sq.download()), info_tuple(gpu_ctx)
        fb.zero(), fb_sq.zero()
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb, 0, 4, framebuffer_sq=fb_sq)
        before = info_tuple(gpu_ctx)
        render.render_features(gpu_ctx, ds, st.camera_settings, st, generate_tiles(W, H, (16, 16)), ft, 0, 8)
        assert info_tuple(gpu_ctx) == before
        assert ft.download().any()
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb, 4, 4, framebuffer_sq=fb_sq)
        assert fb.download().tobytes() == plain[0].tobytes() and fb_sq.download().tobytes() == plain[1].tobytes()
        assert info_tuple(gpu_ctx) == plain_info
    finally:
        fb.close(), fb_sq.close(), ft.close(), ds.close()
