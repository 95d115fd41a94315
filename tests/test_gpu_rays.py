"""rmd_intersect_rays and rmd_camera_rays on the device, against the records tests/rays_ref.py composes from the oracle.

1  Parity, on the ray sets of rays_ref (tests/test_rays_host.py checks each to be what it names).  `object` and `triangle` equal the oracle's; a miss is
   the 40 stated bytes; t is within 4 ulps (the bar tests/test_gpu_grid_walk.py holds this call path to); a plane's normal is its stored bytes; a
   sphere's or a triangle's is within 1e-9 * max(1, |ref|) per component, NaN only for NaN.  On set (a) no ray is left out.  On sets (b) - (d) a ray whose
   object or triangle differs must be fragile by first_hit_ref.fragile_hit, at most 3 of them a batch.  Every set prints its figures as one line.
2  Position independence: a permutation of the rays gives the permuted records byte for byte; the first k rays alone give the first k records and
   leave the records behind them alone; a batch tiled to one ray more than one pass of the launch's waves serves gives the tiled records.
3  The forms: _async then rmd_context_synchronize, _host, and the C++ mirror through `raymond_cli intersect` give the Python call's bytes; one object
   beyond the table limit is RMD_ERR_UNSUPPORTED with the hit buffer untouched.
4  rmd_camera_rays against orc_primary_ray bit for bit (tests/test_gpu_parity.py::test_primary_ray's bar) on the cameras of fov_and_aspect, uv = NULL
   against explicit 0.5s byte for byte, and pick on the stock scenes' frame corners and centre against the oracle's object for that ray.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import first_hit_ref as fr
import oracle_lib as O
import rays_ref as ref
from raymond_amd import abi, probe, render, scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
TUNABLES = (abi.RMD_TUNE_AXIS_PAIRS, abi.RMD_TUNE_MASK_BUDGET)
HIT = render.HIT_DTYPE
FILL = 0xAB  # the byte a hit buffer is filled with where a test asks what a call leaves alone


@pytest.fixture(scope="module")
def ctx(product_lib):
    """A context of this module's own: scenes are created under their cases' tunables."""
    with render.Context(0) as c:
        yield c


def device_scene(ctx, rs_or_scene, tunables=None):
    scene, under = (rs_or_scene.scene, rs_or_scene.tunables) if isinstance(rs_or_scene, ref.RaySet) else (rs_or_scene, tunables or {})
    for k in TUNABLES:
        ctx.set_tunable(k, under.get(k, 0))
    try:
        return render.DeviceScene(ctx, scene)
    finally:
        for k in TUNABLES:
            ctx.set_tunable(k, 0)


def filled(n):
    return np.frombuffer(bytes([FILL]) * (n * HIT.itemsize), dtype=HIT).copy()


def run(ctx, ds, rays, n=None, sync=True, capacity=None):
    """the Python call on device buffers: -> the whole hit buffer (capacity records, filled with FILL before the call)"""
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    capacity = len(rays) if capacity is None else capacity
    with render.RayBuffer(ctx, len(rays)) as d_rays, render.HitBuffer(ctx, capacity) as d_hits:
        d_rays.upload(rays)
        d_hits.upload(filled(capacity))
        render.intersect_rays_dev(ctx, ds, d_rays, d_hits, n=n, sync=sync)
        if not sync:
            ctx.synchronize()
        return d_hits.download()


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def hold_batch(label, scene, osc, rays, got, want, exact):
    """-> (largest ulp distance in t, largest normal deviation over its bar's scale, accounted rays) of one batch; asserts the bars"""
    kinds = ref._kinds(scene)
    assert got.shape == want.shape
    off = np.flatnonzero((got["object"] != want["object"]) | (got["triangle"] != want["triangle"]))
    if exact:
        assert off.size == 0, "%s: object or triangle differs on %d rays, first %d: device (%d, %d), oracle (%d, %d)" % (
            label, off.size, off[0], got["object"][off[0]], got["triangle"][off[0]], want["object"][off[0]], want["triangle"][off[0]])
    assert off.size <= 3, "%s: object or triangle differs on %d rays, first %d" % (label, off.size, off[0])
    for i in off.tolist():
        why = fr.fragile_hit(scene, osc, rays[i], int(want["object"][i]), float(want["t"][i]), int(want["triangle"][i]))
        print("%s: ray %d differs: the oracle's hit (object %d, triangle %d, t %r) is %s" % (label, i, want["object"][i], want["triangle"][i], want["t"][i], why))
        assert why is not None, "%s: ray %d differs from the oracle on a hit that is neither grazing nor tied" % (label, i)
    same = np.ones(len(want), dtype=bool)
    same[off] = False
    g, w = got[same], want[same]
    miss = w["object"] < 0
    assert g[miss].tobytes() == ref.MISS.tobytes() * int(miss.sum()), label + ": a miss is not the 40 stated bytes"
    hit = ~miss
    ulp = int(ref.ulps(g["t"][hit], w["t"][hit]).max(initial=0))
    assert ulp <= 4, "%s: t is %d ulps from the oracle's" % (label, ulp)
    k = kinds[np.maximum(w["object"], 0)]
    plane = hit & (k == 0)
    assert same_bytes(g["normal"][plane], w["normal"][plane]), label + ": a plane's normal is not its stored bytes"
    curved = hit & (k != 0)
    gn, wn = g["normal"][curved], w["normal"][curved]
    assert np.array_equal(np.isnan(gn), np.isnan(wn)), label + ": a NaN normal where the oracle's is not, or the reverse"
    with np.errstate(all="ignore"):
        dev = np.abs(gn - wn) / np.maximum(1.0, np.abs(wn))
    worst = float(np.nanmax(dev, initial=0.0))
    assert worst <= 1e-9, "%s: a normal is %g from the oracle's" % (label, worst)
    return ulp, worst, int(off.size)


def hold_set(ctx, kind, key, exact):
    rs, recs = ref.reference(kind, key)
    osc = O.OracleScene(rs.scene)
    ds = device_scene(ctx, rs)
    entry = {"set": rs.label, "rays": 0, "hits": 0, "max_t_ulps": 0, "max_normal_deviation": 0.0, "accounted_rays": 0}
    try:
        for (label, rays), want in zip(rs.batches, recs):
            got = run(ctx, ds, rays)
            ulp, worst, accounted = hold_batch("%s, batch %s" % (rs.label, label), rs.scene, osc, rays, got, want, exact)
            entry["rays"] += len(rays)
            entry["hits"] += int((want["object"] >= 0).sum())
            entry["max_t_ulps"], entry["max_normal_deviation"] = max(entry["max_t_ulps"], ulp), max(entry["max_normal_deviation"], worst)
            entry["accounted_rays"] += accounted
    finally:
        ds.close()
        print("rays: %s" % json.dumps(entry))


# ---------------------------------------------------------------- 1: parity
@pytest.mark.parametrize("name", ref.ROOMS)
def test_adversarial_rays_in_the_rooms_with_no_ray_left_out(ctx, oracle, name):
    hold_set(ctx, "a", name, exact=True)


KEYS_B = ref.keys_b()


@pytest.mark.parametrize("key", KEYS_B, ids=[fr.feature_key_id(k) for k in KEYS_B])
def test_frame_rays_and_incoherent_rays_of_every_case(ctx, oracle, key):
    hold_set(ctx, "b", key, exact=False)


KEYS_C = ref.keys_c()


@pytest.mark.parametrize("key", KEYS_C, ids=[fr.feature_key_id(k) for k in KEYS_C])
def test_grids_on_the_turn_masks_edge_and_nan_normals(ctx, oracle, key):
    hold_set(ctx, "c", key, exact=False)


@pytest.mark.parametrize("n_objects", ref.TABLES)
def test_object_tables_at_the_lds_edges(ctx, oracle, n_objects):
    sizes, buffered = probe.launch_sizes(probe.MODE_TILES, False), probe.launch_sizes(probe.MODE_TILES_BUFFERED, False)
    below = (64 * 1024 - sizes["wave"]) // sizes["object"]  # the last table below the LDS opt-in
    largest = (sizes["budget"] - buffered["wave"]) // sizes["object"]  # check_render_args: the table beside one wave's area and the sort pool
    assert ref.TABLES == (below, below + 1, largest)
    rs, _ = ref.reference("d", n_objects)
    ds = device_scene(ctx, rs)
    try:
        lds = probe.rays_plan(ds, 1920)["lds"]
        assert (lds <= 64 * 1024) == (n_objects == below) and lds <= sizes["budget"]
    finally:
        ds.close()
    hold_set(ctx, "d", n_objects, exact=False)


# ---------------------------------------------------------------- 2: position independence
POSITION_KEYS = (("mesh", "shared_grid", 0, False, None), ("spheres", "shuffled_room", 1, False, None))  # with a grid, and without


@pytest.mark.parametrize("key", POSITION_KEYS, ids=[fr.feature_key_id(k) for k in POSITION_KEYS])
def test_a_rays_record_does_not_depend_on_its_position(ctx, oracle, key):
    rs, _ = ref.reference("b", key)
    rays = rs.batches[0][1]
    n = len(rays)
    ds = device_scene(ctx, rs)
    try:
        plan = probe.rays_plan(ds, n)
        assert plan["waves_per_wg"] == (4 if key[0] == "mesh" else 1) and plan["batches"] == (n + 63) // 64
        base = run(ctx, ds, rays)
        assert (base["object"] >= 0).any() and len(np.unique(base["object"])) > 3
        # a seeded permutation of the rays: the permuted records
        perm = np.random.default_rng(36).permutation(n)
        assert same_bytes(run(ctx, ds, rays[perm]), base[perm])
        # the first k rays alone: the first k records, and the records behind them keep their bytes
        for k in (1, 63, 64, 65):
            got = run(ctx, ds, rays, n=k)
            assert same_bytes(got[:k], base[:k]) and same_bytes(got[k:], filled(n - k)), k
            short = run(ctx, ds, rays[:k], capacity=k + 70)
            assert same_bytes(short[:k], base[:k]) and same_bytes(short[k:], filled(70)), k
        # tiled to one ray more than one pass of the launch's waves serves: some wave takes a second batch
        waves = probe.rays_plan(ds, abi.RMD_MAX_RAYS)["total_waves"]
        many = waves * 64 + 1
        plan = probe.rays_plan(ds, many)
        assert plan["total_waves"] == waves == plan["batches"] - 1 and waves >= plan["n_cus"] * 64
        reps = -(-many // n)
        tiled = run(ctx, ds, np.tile(rays, (reps, 1))[:many], capacity=many + 3)
        assert same_bytes(tiled[:many], np.tile(base, reps)[:many]) and same_bytes(tiled[many:], filled(3))
    finally:
        ds.close()


# ---------------------------------------------------------------- 3: the forms
@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


FORM_SCENES = {"spheres": scenes.reflective_spheres, "dragon:12": lambda: scenes.gold_dragon_standin(n=12)}


@pytest.mark.parametrize("word", sorted(FORM_SCENES))
def test_every_form_gives_the_same_bytes(ctx, oracle, cli, tmp_path, word):
    scene = FORM_SCENES[word]()
    rays = ref._frame_rays(scene, scenes.camera(40, 24), scenes.SEED, False, 7)
    rays = np.ascontiguousarray(np.concatenate([rays, [[0.0, 0.0, 0.0, np.nan, 0.0, 1.0], [np.inf, 0.0, 0.0, 0.0, 0.0, 1.0], [0.0] * 6]]))
    ds = device_scene(ctx, scene)
    try:
        base = run(ctx, ds, rays)
        want = ref.expected_records(scene, rays)
        assert np.array_equal(base["object"], want["object"]) and (base["object"] >= 0).sum() > 960 and (base["object"][-3:] == -1).all()
        assert same_bytes(run(ctx, ds, rays, sync=False), base)  # _async, then rmd_context_synchronize
        h = render.intersect_rays(ctx, ds, rays)  # _host
        assert same_bytes(h.object.base, base) and np.array_equal(h.t.view(np.uint64), base["t"].view(np.uint64))
    finally:
        ds.close()
    rays.tofile(str(tmp_path / "rays.f64"))
    r = subprocess.run([cli, "intersect", word, "--rays", str(tmp_path / "rays.f64"), "--out", str(tmp_path / "out.hits")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "%d rays, %d hits\n" % (len(rays), int((base["object"] >= 0).sum()))
    assert same_bytes(np.fromfile(str(tmp_path / "out.hits"), dtype=HIT), base)  # the C++ mirror


def test_one_object_beyond_the_table_limit_is_unsupported(ctx, oracle):
    from test_gpu_features_scenes import table_scene

    n = ref.TABLES[-1] + 1
    rays = np.ascontiguousarray(ref.set_d(ref.TABLES[0]).batches[0][1][:130])
    ds = device_scene(ctx, table_scene(n))
    try:
        assert probe.scene_layout(ds)[0] == n
        before = filled(len(rays))
        with render.RayBuffer(ctx, len(rays)) as d_rays, render.HitBuffer(ctx, len(rays)) as d_hits:
            d_rays.upload(rays)
            d_hits.upload(before)
            for fn in (ctx.L.rmd_intersect_rays, ctx.L.rmd_intersect_rays_async):
                assert fn(ctx.handle, ds.handle, d_rays.ptr, len(rays), d_hits.ptr) == abi.RMD_ERR_UNSUPPORTED
                assert b"160 KiB LDS" in ctx.L.rmd_last_error(ctx.handle)
            ctx.synchronize()
            assert same_bytes(d_hits.download(), before)
        host = before.copy()
        status = ctx.L.rmd_intersect_rays_host(ctx.handle, ds.handle, rays.ctypes.data_as(C.c_void_p), len(rays), host.ctypes.data_as(C.c_void_p))
        assert status == abi.RMD_ERR_UNSUPPORTED and same_bytes(host, before)
        other = render.Context(0)  # a scene of another context is refused before it
        try:
            with render.RayBuffer(other, 1) as r1, render.HitBuffer(other, 1) as h1:
                assert other.L.rmd_intersect_rays(other.handle, ds.handle, r1.ptr, 1, h1.ptr) == abi.RMD_ERR_INVALID_ARGUMENT
                assert b"another context" in other.L.rmd_last_error(other.handle)
        finally:
            other.close()
    finally:
        ds.close()


# ---------------------------------------------------------------- 4: rmd_camera_rays
def test_camera_rays_are_the_oracles_primary_rays(ctx, oracle):
    import sphere_scenes as ss

    L = oracle.load()
    rng = np.random.default_rng(37)
    cams = [ss.build(("fov_and_aspect", seed, False))[1] for seed in range(len(ss.FOV_AND_ASPECT))] + [scenes.camera(1920, 1080)]
    assert [(c.backbuffer_width, c.backbuffer_height) for c in cams[:-1]] == [frame for _, frame in ss.FOV_AND_ASPECT]  # narrow and wide, both aspects
    assert min(c.fov_vert for c in cams) < 10.0 and max(c.fov_vert for c in cams) > 120.0
    for cam in cams:
        W, H = cam.backbuffer_width, cam.backbuffer_height
        xy = fr.pixel_grid(W, H)[0] if W * H < 4096 else np.stack([rng.integers(0, W, 4096), rng.integers(0, H, 4096)], axis=1).astype(np.uint32)
        xy = np.ascontiguousarray(np.concatenate([xy, [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]]]).astype(np.uint32))
        uv = rng.uniform(0, 1, (len(xy), 2))
        uv[:8] = [[0.0, 0.0], [1.0, 1.0], [0.5, 0.5], [0.0, 1.0], [2.0**-53, 1.0 - 2.0**-53], [0.25, 0.75], [1.0, 0.0], [0.5, 0.0]]
        c = cam.pod()
        for u in (uv, np.full((len(xy), 2), 0.5)):
            want = np.zeros((len(xy), 6))
            L.orc_primary_ray(len(xy), C.byref(c), oracle.ptr(xy), oracle.ptr(np.ascontiguousarray(u)), oracle.ptr(want))
            with render.camera_rays(ctx, cam, xy, uv=u) as d_rays:
                got = d_rays.download()
            assert ref.ulps(got, want).max() == 0, (W, H)  # tan() is evaluated by the host libm on both sides
        with render.camera_rays(ctx, cam, xy) as d_rays:  # uv = NULL: the explicit 0.5s, byte for byte
            assert same_bytes(d_rays.download(), got)
    # into a buffer of the caller's, whose other rays keep their bytes
    with render.RayBuffer(ctx, 10) as d_rays:
        marks = np.arange(60, dtype=np.float64).reshape(10, 6)
        d_rays.upload(marks)
        render.camera_rays(ctx, cams[-1], [[5, 6], [7, 8]], out=d_rays)
        back = d_rays.download()
        assert same_bytes(back[2:], marks[2:]) and not same_bytes(back[:2], marks[:2])


@pytest.mark.parametrize("word", sorted(FORM_SCENES))
def test_pick_on_the_stock_scenes_corners_and_centre(ctx, oracle, cli, word):
    scene = FORM_SCENES[word]()
    osc = oracle.OracleScene(scene)
    W, H = 64, 48
    cam = scenes.camera(W, H)
    c = cam.pod()
    ds = device_scene(ctx, scene)
    try:
        for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2)):
            xy, u, ray = np.array([[x, y]], dtype=np.uint32), np.full((1, 2), 0.5), np.zeros((1, 6))
            oracle.load().orc_primary_ray(1, C.byref(c), oracle.ptr(xy), oracle.ptr(u), oracle.ptr(ray))
            want = ref.expected_records(scene, ray, osc=osc)[0]
            obj, tri, t, normal = render.pick(ctx, ds, cam, x, y)
            assert (obj, tri) == (int(want["object"]), int(want["triangle"])) and obj >= 0, (x, y)
            assert ref.ulps(np.array([t]), np.array([want["t"]])).max() <= 4 and np.abs(normal - want["normal"]).max() <= 1e-9
    finally:
        ds.close()
    # ... and the C++ mirror's pick prints the same hit in the format its help text defines
    x, y = W // 2, H // 2
    pos = ",".join(repr(float(v)) for v in cam.transform.position)
    r = subprocess.run([cli, "pick", word, "--pixel", "%d,%d" % (x, y), "--size", "%d,%d" % (W, H), "--fov", repr(float(cam.fov_vert)), "--position", pos],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    fields = r.stdout.split()
    assert len(fields) == 6 and r.stdout.endswith("\n") and r.stdout.count("\n") == 1
    assert (int(fields[0]), int(fields[1])) == (obj, tri) and float(fields[2]) == t and [float(v) for v in fields[3:]] == normal.tolist()
