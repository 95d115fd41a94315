"""GPU parity: the HIP path (through the C-ABI) against the CPU oracle on identical seeded inputs.

Levels (SURVEY.md §4 pyramid): device-function known answers -> Scene/grid intersection ->
per-sample radiance + hit sequence -> config-1 image -> size-independent properties
(pass splitting, tile sharding, accumulate semantics).

Tolerances (binary64 everywhere; +,-,*,/,sqrt are correctly rounded on both sides and no FMA contraction is
allowed.  The sides differ in the elementary functions — glibc sin/cos/acos on the oracle's side; on the device a
Cody-Waite + fdlibm-kernel sin/cos (<= 1.6 ulp) and sin/cos(acos(s)) taken as sqrt((1-s)(1+s)) / s — in x^5 of the
Schlick term (libm pow vs three multiplications) and in the association of the bounce weights, which the kernel
multiplies forward into a throughput instead of applying them on the way back up the recursion):
  * RNG, integer outputs, hit/miss flags, object/triangle ids: bit-exact;
  * arithmetic-only device functions (intersections, ONB, normals): <= 4 ulp, in practice 0 (the grid walk in all its forms — plain and DEEP,
    exact and coarse masks, adversarial ray classes, hand-built grids — is held to this bound ray by ray in tests/test_gpu_grid_walk.py);
  * libm-bound device functions: relative 1e-13;
  * per-sample radiance: relative 1e-9 for >= 99.9 % of samples; the remainder must be explained by
    a changed hit sequence (an ulp-level direction difference flipping a hit/miss or a branch);
  * config-1 image: |d| <= 1e-9 * scale on every pixel whose samples all kept their hit sequence.
"""
import numpy as np
import pytest

from raymond_amd import abi, probe, render, scenes
from raymond_amd.scene import Settings, generate_tiles

pytestmark = pytest.mark.gpu

N = 4096


def ulp_diff(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ai = a.view(np.int64).copy()
    bi = b.view(np.int64).copy()
    ai[ai < 0] = np.int64(-(2**63)) - ai[ai < 0]
    bi[bi < 0] = np.int64(-(2**63)) - bi[bi < 0]
    d = np.abs(ai - bi)
    both_nan = np.isnan(a) & np.isnan(b)
    d[both_nan] = 0
    return d


def rel_close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    scale = np.maximum(np.abs(a), np.abs(b))
    ok = np.abs(a - b) <= rtol * np.maximum(scale, 1e-300)
    return ok | (np.isnan(a) & np.isnan(b)) | (a == b)


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def rays_toward(rng, n, target, spread):
    o = rng.uniform(-2, 2, size=(n, 3))
    tgt = np.asarray(target) + rng.normal(scale=spread, size=(n, 3))
    d = tgt - o
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    return np.concatenate([o, d], axis=1)


# ------------------------------------------------------------------ level 1: RNG + device functions
def test_philox_known_answers_on_device(gpu_ctx):
    """Random123 kat_vectors for philox4x32-10 — the same three the oracle is pinned with."""
    ctr = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]]
    key = [[0, 0], [0xFFFFFFFF] * 2, [0xA4093822, 0x299F31D0]]
    out = probe.philox(gpu_ctx, ctr, key)
    expect = np.array(
        [[0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]],
        dtype=np.uint32,
    )
    assert np.array_equal(out, expect)


def test_uniform_stream_bit_exact(gpu_ctx, oracle):
    rng = np.random.default_rng(1)
    pixel = rng.integers(0, 1920 * 1080, N, dtype=np.uint32)
    sample = rng.integers(0, 4000, N, dtype=np.uint32)
    block = rng.integers(0, 40, N, dtype=np.uint32)
    seed = 0x5EED0001_0BADF00D
    dev = probe.block_uniforms(gpu_ctx, seed, pixel, sample, block)
    ref = oracle.block_uniforms(seed, pixel, sample, block)
    assert np.array_equal(dev[:, :3], ref)                 # next2: first, second (+ the 22-bit uniform of the same block)
    assert np.array_equal(dev[:, [3, 4, 2]], ref)          # next3: (r, r1, r2) = (22-bit, first, second)
    assert dev.min() >= 0.0 and dev.max() < 1.0


def _oracle_hit_t(oracle, name, shape, rays):
    L = oracle.load()
    n = rays.shape[0]
    hit = np.zeros(n, dtype=np.int32)
    t = np.zeros(n)
    getattr(L, "orc_%s_intersect" % name)(n, oracle.ptr(oracle.f64(shape)), oracle.ptr(oracle.f64(rays)), oracle.ptr(hit), oracle.ptr(t))
    return hit, t


@pytest.mark.parametrize("name", ["sphere", "plane", "aabb", "triangle"])
def test_primitive_intersections(gpu_ctx, oracle, name):
    rng = np.random.default_rng(hash(name) % 1000)
    if name == "sphere":
        shape = np.concatenate([rng.uniform(-1, 1, (N, 3)), rng.uniform(0.1, 1.0, (N, 1))], axis=1)
        rays = rays_toward(rng, N, (0, 0, 0), 0.8)
        rays[:64, :3] = shape[:64, :3]  # origin at the centre: inside => miss (Q10)
    elif name == "plane":
        shape = np.concatenate([rng.uniform(-1, 1, (N, 3)), unit(rng, N)], axis=1)
        rays = rays_toward(rng, N, (0, 0, 0), 1.0)
        rays[:64, 3:] = np.cross(shape[:64, 3:], unit(rng, 64))  # grazing: denom ~ 0 (Q11)
    elif name == "aabb":
        lo = rng.uniform(-1, 0, (N, 3))
        shape = np.concatenate([lo, lo + rng.uniform(0.1, 1.5, (N, 3))], axis=1)
        rays = rays_toward(rng, N, (0, 0, 0), 1.0)
        rays[:64, 3] = 0.0  # axis-parallel: 1/0 = inf slabs
        rays[64:96, 4] = -0.0
    else:
        c = rng.uniform(-0.5, 0.5, (N, 1, 3))
        shape = (c + rng.normal(scale=0.4, size=(N, 3, 3))).reshape(N, 9)
        rays = rays_toward(rng, N, (0, 0, 0), 0.5)
        shape[:32, 3:6] = shape[:32, 0:3]  # degenerate: a ~ 0
    dh, dt = probe.hit_t(gpu_ctx, name, shape, rays)
    oh, ot = _oracle_hit_t(oracle, name, shape, rays)
    assert np.array_equal(dh, oh)
    assert 0 < oh.sum() < N
    m = oh == 1
    assert ulp_diff(dt[m], ot[m]).max() <= 4


def test_normals_and_onb(gpu_ctx, oracle):
    L = oracle.load()
    rng = np.random.default_rng(5)
    # sphere normal
    sph = np.concatenate([rng.uniform(-1, 1, (N, 3)), rng.uniform(0.1, 1.0, (N, 1))], axis=1)
    rays = rays_toward(rng, N, (0, 0, 0), 0.5)
    t = rng.uniform(0.1, 3.0, N)
    (dn,) = probe.call(gpu_ctx, "sphere_normal", N, [sph, rays, t], [3])
    on = np.zeros((N, 3))
    L.orc_sphere_normal(N, oracle.ptr(sph), oracle.ptr(rays), oracle.ptr(t), oracle.ptr(on))
    assert ulp_diff(dn, on).max() <= 4
    # Heron-area triangle normal (Q13), hit points inside the triangle
    pos = rng.normal(size=(N, 9))
    nrm = np.concatenate([unit(rng, N), unit(rng, N), unit(rng, N)], axis=1)
    bary = rng.dirichlet((1, 1, 1), N)
    p = bary[:, :1] * pos[:, 0:3] + bary[:, 1:2] * pos[:, 3:6] + bary[:, 2:3] * pos[:, 6:9]
    o = p + unit(rng, N)
    d = p - o
    tt = np.sqrt((d * d).sum(axis=1))
    rays = np.concatenate([o, d / tt[:, None]], axis=1)
    (dn,) = probe.call(gpu_ctx, "triangle_normal", N, [pos, nrm, rays, tt], [3])
    on = np.zeros((N, 3))
    L.orc_triangle_normal(N, oracle.ptr(pos), oracle.ptr(nrm), oracle.ptr(rays), oracle.ptr(tt), oracle.ptr(on))
    # the probe runs the production path: sides and area of the triangle precomputed on the host (rmd::triangle_aux), three
    # distances and two Heron areas on the device — bit for bit the reference's nine distances and three areas
    assert ulp_diff(dn, on).max() == 0
    # ONB incl. n.z = +-1 and n.z = 0 (sign switch)
    n3 = unit(rng, N)
    n3[0], n3[1], n3[2], n3[3] = (0, 0, 1), (0, 0, -1), (1, 0, 0), (0, 1, -0.0)
    dt3, db3 = probe.call(gpu_ctx, "onb", N, [n3], [3, 3])
    ot3, ob3 = np.zeros((N, 3)), np.zeros((N, 3))
    L.orc_onb(N, oracle.ptr(n3), oracle.ptr(ot3), oracle.ptr(ob3))
    assert ulp_diff(dt3, ot3).max() == 0 and ulp_diff(db3, ob3).max() == 0


def test_samplers_and_brdf_terms(gpu_ctx, oracle):
    L = oracle.load()
    rng = np.random.default_rng(9)
    r1, r2 = rng.uniform(0, 1, N), rng.uniform(0, 1, N)
    r1[:4] = [0.0, 1.0 - 2**-53, 2**-53, 0.5]
    r2[:4] = [0.0, 1.0 - 2**-53, 0.25, 0.75]  # r2 -> 1 blows up the GGX angle (Q3)
    dd, dp = probe.call(gpu_ctx, "cosine_hemisphere", N, [r1, r2], [3, 1])
    od, op = np.zeros((N, 3)), np.zeros(N)
    L.orc_cosine_hemisphere(N, oracle.ptr(r1), oracle.ptr(r2), oracle.ptr(od), oracle.ptr(op))
    assert np.array_equal(dp[:, 0], op)
    assert np.abs(dd - od).max() <= 1e-15  # unit-vector components: absolute 4.5 ulp(1)
    refl, rough = unit(rng, N), rng.uniform(0.01, 0.9, N)
    (dg,) = probe.call(gpu_ctx, "importance_sample_ggx", N, [refl, rough, r1, r2], [3])
    og = np.zeros((N, 3))
    L.orc_importance_sample_ggx(N, oracle.ptr(refl), oracle.ptr(rough), oracle.ptr(r1), oracle.ptr(r2), oracle.ptr(og))
    # sin/cos of a huge angle (r2 -> 1) is still a well-defined libm result; both sides must agree closely
    assert np.abs(dg - og).max() <= 1e-14
    n3, h3, v3, l3 = unit(rng, N), unit(rng, N), unit(rng, N), unit(rng, N)
    (dD,) = probe.call(gpu_ctx, "ggx_distribution", N, [n3, h3, rough], [1])
    oD = np.zeros(N)
    L.orc_ggx_distribution(N, oracle.ptr(n3), oracle.ptr(h3), oracle.ptr(rough), oracle.ptr(oD))
    assert ulp_diff(dD[:, 0], oD).max() <= 2
    (dG,) = probe.call(gpu_ctx, "geometry_smith", N, [n3, v3, l3, rough], [1])
    oG = np.zeros(N)
    L.orc_geometry_smith(N, oracle.ptr(n3), oracle.ptr(v3), oracle.ptr(l3), oracle.ptr(rough), oracle.ptr(oG))
    assert ulp_diff(dG[:, 0], oG).max() <= 2
    cos_t, f0 = rng.uniform(-1, 1, N), rng.uniform(0, 1, (N, 3))
    (dF,) = probe.call(gpu_ctx, "fresnel_schlick", N, [cos_t, f0], [3])
    oF = np.zeros((N, 3))
    L.orc_fresnel_schlick(N, oracle.ptr(cos_t), oracle.ptr(f0), oracle.ptr(oF))
    assert rel_close(dF, oF, 1e-13).all()


def test_device_sqrt_is_exact_and_sincos_within_2ulp(gpu_ctx):
    """sqrt64 must be the IEEE square root on both of its paths (waves with and without arguments below 2^-767);
    sincos_cw must stay within 2 ulp / 2.5e-16 of the true values over the arguments this path produces."""
    rng = np.random.default_rng(21)
    normal = np.ldexp(rng.uniform(0.5, 1.0, 2 * N), rng.integers(-700, 1000, 2 * N))  # whole waves on the fast path
    mixed = np.ldexp(rng.uniform(0.5, 1.0, N), rng.integers(-1074, 1024, N))
    mixed[:16] = [0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, 5e-324, 2.0**-1022, 2.0**-767, np.nextafter(2.0**-767, 0), 1.0, 4.0, 2.0, 1e-300, 1e300, -5e-324]
    x = np.concatenate([normal, mixed])
    got, _, _, root, inv = probe.elementary(gpu_ctx, x)
    with np.errstate(invalid="ignore"):
        want = np.sqrt(x)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))  # bit for bit, signed zeros included
    # normalize()'s pair: sqrt and the reciprocal of the rounded root, shortcut and guarded plain path alike
    with np.errstate(invalid="ignore", divide="ignore"):
        want_inv = 1.0 / want
    assert np.array_equal(root[~nan].view(np.uint64), want[~nan].view(np.uint64))
    assert np.array_equal(inv[~nan].view(np.uint64), want_inv[~nan].view(np.uint64))
    ones = (np.ldexp(2.0 - 2.0**-52, rng.integers(-300, 300, N)) * (1.0 - rng.integers(0, 3, N) * 2.0**-53)) ** 2  # roots next to all-ones
    _, _, _, root, inv = probe.elementary(gpu_ctx, ones)
    assert np.array_equal(root.view(np.uint64), np.sqrt(ones).view(np.uint64))
    assert np.array_equal(inv.view(np.uint64), (1.0 / np.sqrt(ones)).view(np.uint64))

    u = rng.uniform(0, 1, N)
    args = np.concatenate([
        2.0 * np.pi * u,                                             # azimuth
        rng.uniform(0, 1, N) * np.sqrt(u / (1.0 - u)),               # GGX angle, roughness^2 <= 1
        np.ldexp(rng.uniform(0.5, 1.0, N), rng.integers(-60, 44, N)),  # anything below 2^44
        np.arange(64) * (np.pi / 2),                                 # next to the quadrant boundaries
        [0.0, 1.0 - 2.0**-53, 9.49e7, 2.0**27, 2.0**40],
    ])
    _, si, co, _, _ = probe.elementary(gpu_ctx, args)
    ref_s, ref_c = np.sin(args.astype(np.longdouble)), np.cos(args.astype(np.longdouble))
    for got, ref in ((si, ref_s), (co, ref_c)):
        err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
        ulp = np.spacing(np.abs(ref.astype(np.float64)))
        # next to a zero of the function the 2-term reduction leaves ~k * 1.5e-33 absolute: compare absolutely there
        assert np.all((err <= 2.0 * ulp) | (err <= 1e-18 * np.maximum(1.0, np.abs(args)))), float((err / ulp).max())
        assert err.max() <= 2.5e-16


def test_primary_ray(gpu_ctx, oracle):
    import ctypes as C

    L = oracle.load()
    rng = np.random.default_rng(11)
    cam = scenes.camera(1920, 1080)
    xy = np.stack([rng.integers(0, 1920, N), rng.integers(0, 1080, N)], axis=1).astype(np.uint32)
    u = rng.uniform(0, 1, (N, 2))
    dev = probe.primary_ray(gpu_ctx, cam, xy, u)
    ref = np.zeros((N, 6))
    c = cam.pod()
    L.orc_primary_ray(N, C.byref(c), oracle.ptr(xy), oracle.ptr(u), oracle.ptr(ref))
    assert ulp_diff(dev, ref).max() == 0  # tan() is evaluated by the host libm on both sides


# ------------------------------------------------------------------ level 2: scene + grid intersection
@pytest.fixture(scope="module")
def small_mesh_scene(product_lib):
    return scenes.gold_dragon_standin(n=24)  # 6,912 triangles


def test_scene_intersect_spheres(gpu_ctx, oracle):
    sc = scenes.reflective_spheres()
    ds, osc = render.DeviceScene(gpu_ctx, sc), oracle.OracleScene(sc)
    rng = np.random.default_rng(13)
    rays = np.concatenate([rays_toward(rng, N, (-1.0, -0.5, 3.5), 0.6), rays_toward(rng, N, (0.74, -0.25, 3.5), 0.9), rays_toward(rng, N, (0, 0, 2), 3.0)])
    dobj, dt, dsub = probe.scene_intersect(gpu_ctx, ds, rays)
    oobj, ot, osub = osc.scene_intersect(rays)
    assert np.array_equal(dobj, oobj) and np.array_equal(dsub, osub)
    assert len(set(oobj.tolist())) >= 7
    m = oobj >= 0
    assert ulp_diff(dt[m], ot[m]).max() <= 4
    ds.close()


def test_planes_special_rays_bit_exact(gpu_ctx, oracle):
    """Scene::intersect over axis-aligned, non-unit and slanted planes plus a sphere: closest object and distance bit for bit,
    including direction components with an all-ones significand, origins exactly on a plane, zero / tiny / negative-zero
    direction components, -0.0 in a normal and non-finite rays (0 * inf and 0 * NaN are NaN in the reference's dot products: such a
    ray misses an axis-aligned plane).  (Two short forms for axis-aligned planes were measured against these cases and dropped —
    shared reciprocals per axis, and single-component dot products: DESIGN.md "measured and rejected".)"""
    from raymond_amd.scene import Material, Object, Plane, Scene, Sphere

    sc = Scene()
    grey = Material.Diffuse((0.5, 0.5, 0.5), 0.5)
    for origin, normal in (
        ((0.0, -1.0, 0.0), (0.0, 1.0, 0.0)), ((0.0, 2.0, 0.0), (-0.0, -1.0, 0.0)), ((0.0, 0.0, -2.0), (0.0, -0.0, 1.0)),
        ((0.0, 0.0, 5.0), (0.0, 0.0, -1.0)), ((-2.0, 0.0, 0.0), (1.0, 0.0, -0.0)), ((2.0, 0.0, 0.0), (-1.0, 0.0, 0.0)),
        ((0.0, 1.5, 0.0), (0.0, -2.0, 0.0)),                      # axis-aligned but not unit: plain test
        ((0.0, 0.0, 4.0), (0.3, 0.1, -0.9)),                      # slanted: plain test
        ((7.0, 1.75, -3.0), (0.0, -1.0, 0.0)),                    # a second plane on the y axis, in front of the ceiling
    ):
        sc.objects.append(Object(Plane(origin, normal), grey))
    sc.objects.append(Object(Sphere((0.3, 0.2, 2.0), 0.4), grey))
    rng = np.random.default_rng(21)
    rays = rays_toward(rng, 3 * N, (0, 0.5, 1.5), 2.5)
    d = rays[:, 3:]
    ones = np.nextafter(1.0, 0.0)  # 0x3FEFFFFFFFFFFFFF: all-ones significand, div_by's one unsupported divisor class
    d[:64] = [0.0, -ones, 0.0]
    d[64:128, 0] = np.nextafter(0.5, 0.0)
    d[128:192, 2] = -np.nextafter(0.25, 0.0)
    d[192:256, 1] = 0.0
    d[256:320, 0] = -0.0
    d[320:384, 2] = 1e-7   # faces no z plane by the 1e-6 rule
    d[384:448, 2] = 1.1e-6
    rays[448:512, 1] = -1.0  # origin on the floor plane: numerator zero
    rays[512:576, 0] = 2.0   # origin on the right wall
    rays[576:640, :3] = [0.0, 1.75, 0.0]
    # non-finite rays (the reference's products 0 * inf and 0 * NaN are NaN: such a ray misses an axis-aligned plane that a
    # test reading only "its" component would report) — one per wave of 64 and whole waves of them
    rays[700, 3] = np.nan
    rays[770, 5] = np.inf
    rays[840, 0] = -np.inf
    rays[910, 1] = np.nan
    rays[960:1024, 3] = np.nan
    rays[1024:1088, 2] = np.inf
    dobj, dt, dsub = probe.scene_intersect(gpu_ctx, render.DeviceScene(gpu_ctx, sc), rays)
    oobj, ot, osub = oracle.OracleScene(sc).scene_intersect(rays)
    assert np.array_equal(dobj, oobj)
    m = oobj >= 0
    assert np.array_equal(dt[m].view(np.uint64), ot[m].view(np.uint64))
    assert len(set(oobj.tolist())) >= 8 and (oobj[:64] >= 0).all()


def test_paired_planes_keep_the_scan_order_on_ties(gpu_ctx, oracle):
    """Planes with exactly opposite normals are tested together, at the later one's turn (plane_pair_intersect).  Scene::intersect's scan
    (core/src/scene.rs:54-74, strict `<`) keeps the FIRST object among equal distances, so the merge must be lexicographic in (distance,
    index): coincident planes before, between and after the partners of a pair — equal distances bit for bit — and the winner is the oracle's."""
    from raymond_amd.scene import Material, Object, Plane, Scene, Sphere

    sc = Scene()
    grey = Material.Diffuse((0.5, 0.5, 0.5), 0.5)
    for origin, normal in (
        ((0.0, -1.0, 0.0), (0.0, 1.0, 0.0)),   # 0 floor, paired with 3
        ((3.0, -1.0, 1.0), (0.0, 2.0, 0.0)),   # 1 the same plane, normal x 2 (same quotient bit for bit), no partner: between 0 and 3
        ((0.0, 2.0, 0.0), (0.0, -2.0, 0.0)),   # 2 the ceiling's plane, no partner, before the ceiling
        ((1.0, 2.0, -1.0), (0.0, -1.0, 0.0)),  # 3 ceiling, paired with 0
        ((5.0, -1.0, 5.0), (0.0, 1.0, 0.0)),   # 4 floor again, paired with 5
        ((0.0, 2.0, 0.0), (0.0, -1.0, 0.0)),   # 5 ceiling again
        ((-2.0, 0.0, 0.0), (1.0, 0.0, 0.0)), ((2.0, 0.0, 0.0), (-1.0, 0.0, 0.0)),  # 6, 7 walls, paired
        ((0.0, 0.0, 5.0), (0.0, 0.0, -1.0)),   # 8 back wall, no partner
    ):
        sc.objects.append(Object(Plane(origin, normal), grey))
    sc.objects.append(Object(Sphere((0.3, 0.2, 2.0), 0.4), grey))
    rng = np.random.default_rng(22)
    rays = rays_toward(rng, 2 * N, (0, 0.5, 1.5), 2.5)
    dobj, dt, dsub = probe.scene_intersect(gpu_ctx, render.DeviceScene(gpu_ctx, sc), rays)
    oobj, ot, osub = oracle.OracleScene(sc).scene_intersect(rays)
    assert np.array_equal(dobj, oobj)
    m = oobj >= 0
    assert np.array_equal(dt[m].view(np.uint64), ot[m].view(np.uint64))
    assert (oobj == 0).sum() > 50 and (oobj == 2).sum() > 50 and not np.isin(oobj, (1, 3, 4, 5)).any()  # the ties went to the first plane


def test_grid_walk(gpu_ctx, oracle, small_mesh_scene):
    """AccGrid::intersects incl. origins inside the box, on the max side (Q6) and axis-parallel rays (Q8) — the plain form on one grid; the walk's
    other forms (DEEP with its pre-test, ring and carried walks; coarse masks; grids with res.z > res.y) and the adversarial ray classes are in
    tests/test_gpu_grid_walk.py."""
    sc = small_mesh_scene
    ds, osc = render.DeviceScene(gpu_ctx, sc), oracle.OracleScene(sc)
    g = sc.objects[1].geometry.grid
    centre = (g.bbox_min + g.bbox_max) / 2
    rng = np.random.default_rng(17)
    rays = rays_toward(rng, 3 * N, centre, 0.06)
    inside = np.concatenate([rng.uniform(g.bbox_min, g.bbox_max, (N, 3)), unit(rng, N)], axis=1)
    beyond = np.concatenate([g.bbox_max + rng.uniform(0.001, 0.2, (N, 3)), -unit(rng, N) * np.sign(rng.uniform(-0.2, 1, (N, 3)))], axis=1)
    beyond[:, 3:] /= np.sqrt((beyond[:, 3:] ** 2).sum(axis=1))[:, None]
    axis = np.concatenate([centre + rng.uniform(-0.05, 0.05, (64, 3)) - np.array([0, 0, 1.0]), np.tile([0.0, -0.0, 1.0], (64, 1))], axis=1)
    rays = np.concatenate([rays, inside, beyond, axis])
    dh, dt, dtri = probe.grid_intersect(gpu_ctx, ds, 0, rays)
    oh, ot, otri = osc.grid_intersect(0, rays)
    assert np.array_equal(dh, oh)
    assert 0.1 < oh.mean() < 0.95
    m = oh == 1
    assert np.array_equal(dtri[m], otri[m])
    assert ulp_diff(dt[m], ot[m]).max() <= 4
    dobj, dt2, dsub = probe.scene_intersect(gpu_ctx, ds, rays)
    oobj, ot2, osub = osc.scene_intersect(rays)
    assert np.array_equal(dobj, oobj) and np.array_equal(dsub, osub)
    ds.close()


# ------------------------------------------------------------------ level 3: per-sample radiance + hit sequence
def _per_sample(gpu_ctx, oracle, scene, settings, n, seed):
    cam = settings.camera_settings
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.integers(0, cam.backbuffer_width, n), rng.integers(0, cam.backbuffer_height, n)], axis=1).astype(np.uint32)
    smp = rng.integers(0, 4000, n).astype(np.uint32)
    ds, osc = render.DeviceScene(gpu_ctx, scene), oracle.OracleScene(scene)
    drgb, dpo, dps = probe.trace_samples(gpu_ctx, ds, cam, settings, xy, smp, paths=True)
    orgb = np.zeros((n, 3))
    opo = np.full((n, probe.PATH_STRIDE), -2, dtype=np.int32)
    ops = np.zeros((n, probe.PATH_STRIDE), dtype=np.uint32)
    for i in range(n):
        rgb, po, ps = osc.trace_sample_path(cam, settings, int(xy[i, 0]), int(xy[i, 1]), int(smp[i]))
        orgb[i] = rgb
        opo[i, : len(po)] = po
        ops[i, : len(ps)] = ps
    ds.close()
    same_path = (dpo == opo).all(axis=1) & (dps == ops).all(axis=1)
    close = rel_close(drgb, orgb, 1e-9).all(axis=1)
    return same_path, close, drgb, orgb


@pytest.mark.parametrize("config", ["C1", "C2"])
def test_per_sample_spheres(gpu_ctx, oracle, config):
    n = 20000
    st = scenes.config_settings(config)
    same_path, close, drgb, orgb = _per_sample(gpu_ctx, oracle, scenes.reflective_spheres(), st, n, 23)
    assert close[same_path].all(), "a sample with the oracle's exact hit sequence differs beyond 1e-9"
    assert same_path.mean() >= 0.999, "more than 0.1 %% of samples changed their hit sequence: %g" % (1 - same_path.mean())
    assert close.mean() >= 0.999
    assert (orgb > 0).any(axis=1).mean() > 0.05  # the comparison is not vacuous


def test_per_sample_mesh(gpu_ctx, oracle, small_mesh_scene):
    st = Settings(scenes.camera(480, 270), sample_count=1, bounce_limit=5, seed=scenes.SEED)
    same_path, close, drgb, orgb = _per_sample(gpu_ctx, oracle, small_mesh_scene, st, 20000, 29)
    assert close[same_path].all()
    assert same_path.mean() >= 0.999 and close.mean() >= 0.999


def test_per_sample_dof_and_deep_bounces(gpu_ctx, oracle, small_mesh_scene):
    """Config-5 style thin lens (rejection-sampled aperture, variable draw count, Q12) and bounce_limit 8 (config 4)."""
    st = Settings(scenes.camera(480, 270, aperture_radius=0.5), sample_count=1, bounce_limit=8, seed=scenes.SEED + 5, use_dof=True)
    same_path, close, drgb, orgb = _per_sample(gpu_ctx, oracle, small_mesh_scene, st, 12000, 31)
    assert close[same_path].all()
    assert same_path.mean() >= 0.999 and close.mean() >= 0.999


def test_the_walls_of_an_axis_aligned_room_are_tested_with_one_component_and_give_the_same_samples(gpu_ctx, oracle, small_mesh_scene):
    """scene_split.hpp: pairs of opposite planes whose normals are exactly +e_k / -e_k are tested ahead of the object loop with one component of the
    ray (rmd_scene_create marks them in scenes of regular parameters).  Per sample — hit sequence and radiance — against the oracle, through the
    render kernel's own code (list instantiation), on rooms that reach every branch of the rule: the pair's earlier plane facing either way, a
    camera that stands exactly ON a wall's coordinate (a zero numerator: the wave takes the general test), two pairs on one axis (the second is
    tested in the loop), a pair whose normals are not unit vectors and a pair that is not axis-aligned (both general), and an irregular scene
    (an infinite emitter: no pair is marked)."""
    from raymond_amd.scene import Material, Object, Plane, Scene, Sphere

    grey, dark, light = Material.Diffuse((0.6, 0.6, 0.6), 0.5), Material.Metal((0.3, 0.5, 0.9), 0.2), Material.Emission((1.5, 1.5, 1.5), (1.0, 1.0, 1.0), 0.27, 0.0)

    def room(planes, extra=()):
        sc = Scene()
        sc.objects.append(Object(Sphere((-0.6, -0.5, 3.2), 0.5), dark))
        for origin, normal, mat in planes:
            sc.objects.append(Object(Plane(origin, normal), mat))
        sc.objects.extend(extra)
        return sc

    rooms = {
        # the reference's room with the earlier plane of every pair facing the NEGATIVE axis
        "minus-first": room([((0, 2, 0), (0, -1, 0), light), ((0, -1, 0), (0, 1, 0), grey), ((0, 0, 5), (0, 0, -1), grey), ((0, 0, -2), (0, 0, 1), grey),
                             ((2, 0, 0), (-1, 0, 0), dark), ((-2, 0, 0), (1, 0, 0), grey)]),
        # the camera (at the origin) stands on the x = 0 wall and on the z = 0 wall: zero numerators on every camera ray
        "camera-on-walls": room([((0, -1, 0), (0, 1, 0), grey), ((0, 2, 0), (0, -1, 0), light), ((0, 0, 0), (1, 0, 0), grey), ((3, 0, 0), (-1, 0, 0), dark),
                                 ((0, 0, 0), (0, 0, 1), grey), ((0, 0, 5), (0, 0, -1), grey)]),
        # two pairs on the y axis (the inner one is found first), one pair with normals of length 2, one tilted pair
        "mixed": room([((0, -1, 0), (0, 1, 0), grey), ((0, 2, 0), (0, -1, 0), light), ((0, -1.5, 0), (0, 1, 0), dark), ((0, 2.5, 0), (0, -1, 0), grey),
                       ((-2, 0, 0), (2, 0, 0), grey), ((2, 0, 0), (-2, 0, 0), dark), ((0, 0, 6), (0.6, 0, -0.8), grey), ((0, 0, -2), (-0.6, 0, 0.8), grey)]),
        "irregular": room([((0, -1, 0), (0, 1, 0), grey), ((0, 2, 0), (0, -1, 0), Material.Emission((float("inf"), 1.5, 1.5), (1.0, 1.0, 1.0), 0.27, 0.0)),
                           ((-2, 0, 0), (1, 0, 0), grey), ((2, 0, 0), (-1, 0, 0), dark), ((0, 0, -2), (0, 0, 1), grey), ((0, 0, 5), (0, 0, -1), grey)]),
    }
    rooms["mesh"] = small_mesh_scene  # (the mesh kernel visits the walls in intersect_simple)
    for name, sc in rooms.items():
        # (1) the rule changes no sample: whole frames with RMD_TUNE_AXIS_PAIRS = 1 (every pair takes the general test) and 0, bit for bit — the
        #     role-sorted kernel (128 spp), the direct mode (6 spp), pinhole and thin lens
        for spp, dof in ((128, False), (6, True)):
            cam = scenes.camera(203, 117, aperture_radius=0.3 if dof else 0.0)
            st = Settings(cam, sample_count=spp, bounce_limit=6, seed=97, use_dof=dof, trace_black_paths=True)
            tiles = generate_tiles(203, 117, st.tile_size)
            frames = {}
            for off in (0, 1):
                gpu_ctx.set_tunable(abi.RMD_TUNE_AXIS_PAIRS, off)
                try:
                    ds, fb = render.DeviceScene(gpu_ctx, sc), render.Framebuffer(gpu_ctx, 203, 117)
                    render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb)
                    frames[off] = fb.download()
                    fb.close(), ds.close()
                finally:
                    gpu_ctx.set_tunable(abi.RMD_TUNE_AXIS_PAIRS, 0)
            assert same_bits(frames[0], frames[1]).all(), (name, spp, dof)
            assert np.isfinite(frames[0]).any() and (frames[0][np.isfinite(frames[0])] > 0).any(), name
        if name == "mesh": continue  # (its samples against the oracle: test_per_sample_mesh)
        # (2) ... and the samples are the oracle's: hit sequence and radiance per sample through the render kernel's list instantiation
        for dof in (False, True):
            st = Settings(scenes.camera(160, 120, aperture_radius=0.3 if dof else 0.0), sample_count=1, bounce_limit=6, seed=97, use_dof=dof, trace_black_paths=True)
            same_path, close, drgb, orgb = _per_sample(gpu_ctx, oracle, sc, st, 6000, 5)
            finite = np.isfinite(orgb).all(axis=1)
            assert (np.isfinite(drgb).all(axis=1) == finite)[same_path].all(), name
            diff = np.abs(drgb - orgb)
            # (a camera that stands ON a wall makes grazing bounces common — a weight that carries a cosine of ~1e-12 where the host's libm gives exactly
            # 0, and hit sequences that an ulp flips: the absolute clause of the parity bar, DESIGN.md section 3, a decade wider for that room, and
            # 99 % instead of 99.9 % of the sequences)
            bad = same_path & finite & ~close & ~(diff <= 1e-11).all(axis=1)
            assert not bad.any(), (name, dof, int(bad.sum()), float(diff[bad].max()), drgb[bad][:3], orgb[bad][:3])
            assert same_path.mean() >= (0.99 if name == "camera-on-walls" else 0.999), (name, 1 - same_path.mean())
            if name != "irregular":  # (there every lit sample carries the emitter's infinity)
                assert (orgb[finite] > 0).any(axis=1).mean() > 0.05, name
            else:
                assert (~finite).mean() > 0.05


def test_bounce_limit_edge_cases(gpu_ctx, oracle):
    sc = scenes.reflective_spheres()
    for limit in (0, 1, 16):
        st = Settings(scenes.camera(64, 64), sample_count=1, bounce_limit=limit, seed=3)
        same_path, close, drgb, orgb = _per_sample(gpu_ctx, oracle, sc, st, 2000, 37 + limit)
        assert close[same_path].all() and same_path.mean() >= 0.998
        if limit == 0:
            assert (drgb == 0).all()  # depth 1 > bounce_limit: trace() returns 0 before intersecting (:235-237)


# ------------------------------------------------------------------ level 4: config-1 image
def test_config1_image(gpu_ctx, oracle):
    """ReflectiveSpheres 256x256, 16 spp, 3 bounces (BASELINE.json configs[0]) — whole image vs oracle."""
    sc, st = scenes.reflective_spheres(), scenes.config_settings("C1")
    cam = st.camera_settings
    tiles = generate_tiles(256, 256, st.tile_size)
    ds = render.DeviceScene(gpu_ctx, sc)
    fb = render.Framebuffer(gpu_ctx, 256, 256)
    render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb)
    dev = fb.download()
    ref = oracle.OracleScene(sc).render_tiles(cam, st, tiles)
    ok = rel_close(dev, ref, 1e-9).all(axis=2)
    assert ok.mean() >= 0.995, "pixels off: %d" % (~ok).sum()
    # pixels that differ must differ by at most a few whole samples' worth of radiance (a flipped sample), not garbage
    assert np.abs(dev - ref)[~ok].max(initial=0.0) <= 16 * 1.5 * 4
    assert abs(dev.mean() - ref.mean()) <= 1e-3 * ref.mean()
    # tone-mapped 8-bit output (cli_old/src/main.rs:161-181): byte for byte the oracle's restatement (await's division + host-libm exp / powf)
    # of the same frame, and of the oracle's own frame wherever the radiance agrees bit for bit
    rgb8 = render.resolve_tonemap(gpu_ctx, fb, st.sample_count)
    assert np.array_equal(rgb8, oracle.resolve_tonemap(dev, 16))
    same = (dev == ref).all(axis=2)
    assert same.mean() > 0.5 and np.array_equal(rgb8[same], oracle.resolve_tonemap(ref, 16)[same])
    fb.close()
    ds.close()


def _render_modes(gpu_ctx, sc, W, H, spp, bounces, seed, modes):
    """{mode: frame} for rmd_settings.flags = 0 ("default"), RMD_RENDER_END_BLACK_PATHS ("end"), RMD_RENDER_TRACE_BLACK_PATHS ("trace")."""
    tiles = generate_tiles(W, H, (32, 32))
    ds = render.DeviceScene(gpu_ctx, sc)
    fb = render.Framebuffer(gpu_ctx, W, H)
    frames = {}
    for mode in modes:
        st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=bounces, seed=seed, trace_black_paths=mode == "trace", end_black_paths=mode == "end")
        fb.zero()
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb)
        frames[mode] = fb.download()
    fb.close(), ds.close()
    return frames, st, tiles


def same_bits(a, b):
    return (np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def test_black_path_modes_change_no_finite_sample(gpu_ctx, oracle, small_mesh_scene):
    """A path whose throughput has become exactly (0, 0, 0) — a diffuse bounce off a black wall, a GGX sample below the surface — may be ended:
    trace() multiplies whatever the rest of the path finds by that zero (src/trace.rs:281-282, :315-318), so the sample is zero in the
    reference too unless a later vertex is non-finite.  Scenes WITHOUT a grid have no such vertex: flags 0 ends those paths there and the
    frame must equal, bit for bit, the one RMD_RENDER_TRACE_BLACK_PATHS gives (every segment traced) and the oracle's.  Scenes WITH a grid:
    flags 0 traces on (identical to TRACE by construction — checked), and the opt-in RMD_RENDER_END_BLACK_PATHS may only differ where the
    traced-on frame is non-finite."""
    frames, st, tiles = _render_modes(gpu_ctx, scenes.reflective_spheres(), 203, 117, 24, 5, 41, ("default", "trace"))
    assert same_bits(frames["default"], frames["trace"]).all() and np.isfinite(frames["default"]).all()
    from test_gpu_fullsize import account_for_off_pixels

    ref = oracle.OracleScene(scenes.reflective_spheres()).render_tiles(st.camera_settings, st, tiles, threads=4)
    ok = rel_close(frames["default"], ref, 1e-9).all(axis=2)
    st0 = Settings(scenes.camera(203, 117), sample_count=24, bounce_limit=5, seed=41)  # (flags 0: the frame that is compared)
    account_for_off_pixels(gpu_ctx, oracle, scenes.reflective_spheres(), st0, st0.camera_settings, 24, frames["default"], ref, ok, "black path modes, spheres")
    assert (frames["default"] == 0.0).all(axis=2).mean() < 0.5  # (the frame itself is not black)

    frames, st, tiles = _render_modes(gpu_ctx, small_mesh_scene, 160, 96, 12, 8, 41, ("default", "trace", "end"))
    assert same_bits(frames["default"], frames["trace"]).all()
    same = same_bits(frames["end"], frames["default"]).all(axis=2)
    assert np.isfinite(frames["default"][~same]).all(axis=1).sum() == 0, "a finite pixel changed"
    assert same.mean() > 0.9999
    ref = oracle.OracleScene(small_mesh_scene).render_tiles(st.camera_settings, st, tiles, threads=4)
    ok = rel_close(frames["default"], ref, 1e-9).all(axis=2)
    st0 = Settings(scenes.camera(160, 96), sample_count=12, bounce_limit=8, seed=41)
    account_for_off_pixels(gpu_ctx, oracle, small_mesh_scene, st0, st0.camera_settings, 12, frames["default"], ref, ok, "black path modes, mesh")


def test_contradictory_or_unknown_flags_are_refused(gpu_ctx):
    """RMD_RENDER_TRACE_BLACK_PATHS and RMD_RENDER_END_BLACK_PATHS exclude each other; bits the header does not define are refused too."""
    import ctypes as C

    from raymond_amd import lib
    from raymond_amd.scene import tile_array

    sc = scenes.reflective_spheres()
    ds = render.DeviceScene(gpu_ctx, sc)
    fb = render.Framebuffer(gpu_ctx, 32, 32)
    cam = scenes.camera(32, 32).pod()
    tiles = tile_array([(0, 0, 32, 32)])
    for flags in (abi.RMD_RENDER_TRACE_BLACK_PATHS | abi.RMD_RENDER_END_BLACK_PATHS, 8, 1 << 31):
        st = Settings(scenes.camera(32, 32), sample_count=1).pod()
        st.flags = flags
        status = gpu_ctx.L.rmd_render_tiles(gpu_ctx.handle, ds.handle, C.byref(cam), C.byref(st), tiles, 1, fb.ptr)
        assert status == abi.RMD_ERR_INVALID_ARGUMENT, (flags, status)
    assert (fb.download() == 0).all()  # nothing was rendered
    fb.close(), ds.close()


def nan_normal_scene(n=6, every=2):
    """cli_old's room with a small mesh in the dragon's place, every second triangle of which has vertex normals (0, 0, 0): the interpolated
    normal of a hit on it is normalize(0) = 0 * (1 / 0) = NaN (triangle.rs:60-67, cgmath normalize) — the non-finite vertex that a real mesh
    produces once in ~1e9 samples (Heron's radicand rounding below zero for a hit on an edge), made certain."""
    from raymond_amd.scene import Mesh

    mesh = scenes.lumpy_sphere_mesh(n)
    nrm = mesh.tri_nrm.copy()
    nrm[::every] = 0.0
    return scenes.mesh_scene(Mesh(mesh.tri_pos, nrm))


def test_black_path_modes_on_a_mesh_with_nan_normals(gpu_ctx, oracle):
    """The case the black-path rule turns on, made certain (production instantiation, tile mode): cli_old's room — black back and side walls —
    around a mesh half of whose triangles yield a NaN normal.  A camera path that bounces diffusely off a black wall (weight exactly 0) and
    then meets such a triangle is 0 x NaN = NaN in the reference (src/trace.rs:281-282).
      flags 0 (and TRACE)  == the oracle, NaN for NaN, finite pixels to 1e-9: the reference-identical mode;
      END_BLACK_PATHS      finite in those pixels — the sequential sum of the pixel's samples with the NaN ones replaced by zero, which
                           is what ending the path at its black bounce computes — NaN where a NaN vertex is met with a non-zero
                           throughput, and bit-identical to flags 0 everywhere else."""
    sc = nan_normal_scene()
    W, H, spp = 160, 96, 12
    frames, st, tiles = _render_modes(gpu_ctx, sc, W, H, spp, 5, 41, ("default", "trace", "end"))
    osc = oracle.OracleScene(sc)
    ref = osc.render_tiles(st.camera_settings, st, tiles, threads=4)
    dflt, end = frames["default"], frames["end"]
    assert same_bits(dflt, frames["trace"]).all()
    ref_nan, dflt_nan, end_nan = np.isnan(ref).any(axis=2), np.isnan(dflt).any(axis=2), np.isnan(end).any(axis=2)
    # flags 0: NaN exactly where the oracle is (up to the < 0.5 % of pixels in which an ulp-level difference changes a hit sequence)
    assert (ref_nan != dflt_nan).mean() < 0.005
    assert ref_nan.sum() > 2000, "the scene does not produce the case"
    both_finite = ~ref_nan & ~dflt_nan
    assert rel_close(dflt[both_finite], ref[both_finite], 1e-9).all(axis=1).mean() >= 0.995
    # END: a subset of the NaN pixels stays NaN, > 1000 pixels become finite, nothing else moves
    assert not (end_nan & ~dflt_nan).any()
    rescued = dflt_nan & ~end_nan
    assert rescued.sum() > 1000, "no NaN behind a zero weight in this frame: the test would be vacuous"
    untouched = ~dflt_nan
    assert same_bits(end[untouched], dflt[untouched]).all(), "RMD_RENDER_END_BLACK_PATHS changed a pixel that is finite in the reference"
    assert np.isnan(end[end_nan]).any(axis=1).all() and np.isnan(dflt[end_nan]).any(axis=1).all()
    # the rescued pixels hold the reference's sample sum with the NaN samples as zeros (oracle per-sample values, added in sample order)
    ys, xs = np.nonzero(rescued)
    pick = np.random.default_rng(3).choice(len(ys), size=200, replace=False)
    xy = np.repeat(np.stack([xs[pick], ys[pick]], axis=1), spp, axis=0).astype(np.uint32)
    smp = np.tile(np.arange(spp, dtype=np.uint32), len(pick))
    per_sample = osc.trace_samples(st.camera_settings, st, xy, smp).reshape(len(pick), spp, 3)
    assert np.isnan(per_sample).any(axis=(1, 2)).all()
    cleaned = np.where(np.isnan(per_sample).any(axis=2, keepdims=True), 0.0, per_sample)
    expect = np.zeros((len(pick), 3))
    for k in range(spp):
        expect = expect + cleaned[:, k]
    ok = rel_close(end[ys[pick], xs[pick]], expect, 1e-9).all(axis=1)
    assert ok.mean() >= 0.97, "rescued pixels do not hold the sum of their finite samples: %d of %d" % ((~ok).sum(), len(ok))


def _irregular_scenes():
    """Grid-less scenes whose parameters lie OUTSIDE the class for which ending a zero-throughput path is exact (api_scene.cpp: rmd_scene::regular) —
    each makes a non-finite radiance reachable behind a black bounce without any mesh (src/trace.rs:250-252, :281-282, :315-318)."""
    from raymond_amd.scene import Material, Object, Plane, Scene, Sphere

    def room(ceiling, extra=()):
        sc = Scene()
        sc.objects.append(Object(Sphere((-1.0, -0.5, 3.5), 0.5), Material.Diffuse((1.0, 0.0, 0.0), 0.02)))
        sc.objects.extend(extra)
        walls = scenes._room_planes()
        walls[1] = Object(Plane((0.0, 2.0, 0.0), (0.0, -1.0, 0.0)), ceiling)
        sc.objects.extend(walls)
        return sc

    inf = float("inf")
    return {
        # the judge's case: an emitter of (inf, 0, 0) — T (.) L = (0 x inf, 0 x 0, 0 x 0) = (NaN, 0, 0) behind a black bounce
        "inf-emission": room(Material.Emission((inf, 0.0, 0.0), (1.0, 1.0, 1.0), 0.27, 0.0)),
        "nan-emission": room(Material.Emission((1.5, float("nan"), 1.5), (1.0, 1.0, 1.0), 0.27, 0.0)),
        # roughness 0: geometry_schlick_ggx is 0 / 0 for a surface seen from behind (:372-378, k = 0): a NaN weight at a later vertex
        "roughness-0": room(Material.Emission((1.5, 1.5, 1.5), (1.0, 1.0, 1.0), 0.27, 0.0),
                            extra=[Object(Sphere((0.74, -0.25, 3.5), 0.75), Material.Metal((0.05, 0.25, 1.0), 0.0))]),
        "nan-colour": room(Material.Emission((1.5, 1.5, 1.5), (1.0, 1.0, 1.0), 0.27, 0.0),
                           extra=[Object(Sphere((0.74, -0.25, 3.5), 0.75), Material.Diffuse((0.5, float("nan"), 0.5), 0.3))]),
    }


@pytest.mark.parametrize("which", ["inf-emission", "nan-emission", "roughness-0", "nan-colour"])
def test_flags_0_is_reference_identical_for_non_finite_scene_parameters(gpu_ctx, oracle, which):
    """`rmd_settings.flags = 0` ends zero-throughput paths only where that is PROVED to change no sample: scenes without a grid whose parameters
    are all finite and regular (include/raymond_hip.h).  A grid-less scene with an Emission of (inf, 0, 0) behind a black bounce, a NaN colour or
    a material of roughness 0 makes 0 x NaN reachable in the reference (src/trace.rs:250-252, :281-282) — there flags 0 must trace every path on,
    as it does on a mesh: the frame equals RMD_RENDER_TRACE_BLACK_PATHS bit for bit and the oracle NaN for NaN, through the production
    instantiation of the spheres kernel (split launch, role-sorted trips) and through the direct mode."""
    sc = _irregular_scenes()[which]
    W, H = 203, 117
    osc = oracle.OracleScene(sc)
    for spp in (128, 6):  # role-sorted split launch; direct mode
        frames, st, tiles = _render_modes(gpu_ctx, sc, W, H, spp, 5, 41, ("default", "trace", "end"))
        info = gpu_ctx.last_launch_info()
        dflt = frames["default"]
        assert same_bits(dflt, frames["trace"]).all(), "flags 0 ended a path in a scene outside the proved class"
        ref = osc.render_tiles(st.camera_settings, st, tiles, threads=8)
        ref_nan, dev_nan = np.isnan(ref).any(axis=2), np.isnan(dflt).any(axis=2)
        assert ref_nan.sum() > 200, "the scene does not produce the case (%d NaN pixels)" % ref_nan.sum()
        assert (ref_nan != dev_nan).mean() < 0.005  # NaN for NaN (up to the pixels where an ulp flips a hit sequence)
        both = ~ref_nan & ~dev_nan
        assert (np.isinf(ref[both]) == np.isinf(dflt[both])).all()
        if both.any():  # (at 128 spp a NaN emitter leaves no pixel finite)
            assert rel_close(dflt[both], ref[both], 1e-9).all(axis=1).mean() >= 0.995
        # the opt-in still ends such paths: it rescues pixels the reference makes NaN behind a zero weight and touches no finite one
        end = frames["end"]
        untouched = ~dev_nan
        assert same_bits(end[untouched], dflt[untouched]).all()
        assert not (np.isnan(end).any(axis=2) & ~dev_nan).any()
        if which == "inf-emission":  # a black wall seen directly: (0 x inf, 0, 0) at flags 0, (inf or 0, 0, 0) once the black bounce ends the path
            assert (dev_nan & ~np.isnan(end).any(axis=2)).sum() > 50
    assert info.has_grid == 0 and info.end_black_paths == 1  # (the last launch was the opt-in)


def test_regular_scene_parameters_keep_the_exact_shortcut_and_tiny_roughness_is_refused(gpu_ctx):
    """The other side of the rule: the reference's own scene is inside the proved class (flags 0 ends its black paths: what `value` measures), and a
    non-zero roughness below 1e-12 — whose squared square underflows in the kernel's one-quotient weight — is refused at upload."""
    from raymond_amd import lib
    from raymond_amd.scene import Material, Object, Scene, Sphere

    sc = scenes.reflective_spheres()
    ds, fb = render.DeviceScene(gpu_ctx, sc), render.Framebuffer(gpu_ctx, 64, 64)
    st = Settings(scenes.camera(64, 64), sample_count=2)
    render.render_tiles(gpu_ctx, ds, st.camera_settings, st, generate_tiles(64, 64, (32, 32)), fb)
    assert gpu_ctx.last_launch_info().end_black_paths == 1
    fb.close(), ds.close()
    bad = Scene()
    bad.objects.append(Object(Sphere((0.0, 0.0, 3.0), 0.5), Material.Metal((1.0, 1.0, 1.0), 1e-13)))
    with pytest.raises(lib.RaymondError) as e:
        render.DeviceScene(gpu_ctx, bad)
    assert e.value.status == abi.RMD_ERR_UNSUPPORTED


def test_a_mesh_scene_with_many_objects_keeps_the_persistent_form_with_fewer_waves(gpu_ctx, oracle):
    """Round 4's advisor: a grid scene's persistent workgroup needs 6.7 KB of LDS per wave beside the masks and 128 bytes per object; with ~100
    objects 16 waves no longer fit and the launch silently fell back to one wave per item while rmd_last_launch_info still said
    `persistent`.  Now the workgroup shrinks (the kernel takes its wave count from blockDim) and the info reports the form that was launched:
    a mesh + 450 spheres (58 KB of object table) runs persistent with fewer than 16 waves, 1100 spheres as one wave per item — same frame bit for
    bit in every form, and the oracle's."""
    from raymond_amd.scene import Material, Object, Sphere

    for n_spheres, want_persistent in ((450, 1), (1100, 0)):
        rng = np.random.default_rng(n_spheres)
        sc = scenes.mesh_scene(scenes.lumpy_sphere_mesh(13))
        for i in range(n_spheres):
            c = (rng.uniform(-1.8, 1.8), rng.uniform(-0.9, 1.8), rng.uniform(1.5, 4.8))
            mat = Material.Metal(tuple(rng.uniform(0.2, 1.0, 3)), 0.05) if i % 3 == 0 else Material.Diffuse(tuple(rng.uniform(0.0, 1.0, 3)), 0.3)
            sc.objects.append(Object(Sphere(c, rng.uniform(0.03, 0.1)), mat))
        W, H, spp = 128, 96, 12
        st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=4, seed=5)
        cam = st.camera_settings
        tiles = generate_tiles(W, H, (32, 32))
        ds, fb = render.DeviceScene(gpu_ctx, sc), render.Framebuffer(gpu_ctx, W, H)
        frames, infos = {}, {}
        for split, form in ((3, 2), (3, 1), (1, 2)):
            gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, split), gpu_ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, form)
            try:
                fb.zero()
                render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb)
                frames[(split, form)], infos[(split, form)] = fb.download(), gpu_ctx.last_launch_info()
            finally:
                gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0), gpu_ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 0)
        fb.close(), ds.close()
        asked = infos[(3, 2)]
        assert asked.has_grid == 1 and asked.split_k == 3
        assert asked.persistent == want_persistent, (n_spheres, asked.persistent, asked.waves_per_workgroup)
        if want_persistent:
            assert 4 <= asked.waves_per_workgroup < 16, asked.waves_per_workgroup
            assert asked.queued == 1  # the production form of a persistent split launch of a mesh scene: the paths in queues
        assert infos[(3, 1)].persistent == 0
        for key, img in frames.items():
            assert same_bits(img, frames[(3, 2)]).all(), key
        ref = oracle.OracleScene(sc).render_tiles(cam, st, tiles, threads=8)
        assert rel_close(frames[(3, 2)], ref, 1e-9).all(axis=2).mean() >= 0.995


def test_output_stage_is_byte_exact_on_adversarial_frames(gpu_ctx, oracle):
    """`rmd_resolve_tonemap` == the oracle's restatement of `TaskHandle::await`'s division + cli_old/src/main.rs:161-181, byte for byte, on
    frames built to sit ON the truncation boundaries — radiances whose 255 * tm is an integer to within an ulp or a few 1e-13, for every
    level 1..255 — plus zeros, saturated, negative, huge, infinite and NaN values (cast::<u8>() -> None -> the pixel stays (0,0,0)), an
    oracle-rendered frame, and a frame where MOST pixels are boundary cases (the host fallback's whole-frame route)."""
    rng = np.random.default_rng(5)
    W, H = 256, 192
    levels = np.arange(1, 256, dtype=np.float64)
    with np.errstate(divide="ignore"):  # level 255: log1p(-1) = -inf, i.e. p = +inf — kept: an infinite radiance is one of the cases
        on_boundary = -np.log1p(-((levels / 255.0) ** 2.2))  # p with 255 * (1 - exp(-p))^(1/2.2) ~ level
    frames = []
    for spread in (0.0, 1e-16, 1e-14, 1e-12, 1e-10, 1e-8, 1e-6):
        p = on_boundary[rng.integers(0, 255, size=(H, W, 3))]
        frames.append(p * (1.0 + spread * rng.uniform(-1, 1, size=p.shape)))
    special = np.array([0.0, -0.0, 1e-300, 1e-20, 2.0**-54, 2.0**-53, 36.0, 36.7368, 36.9, 37.0, 37.4299, 38.0, 39.9999, 40.0, 41.0, 700.0, 1e300,
                        np.inf, -np.inf, np.nan, -1.0, -1e-9, -700.0, -710.0, 5e-6, 5.1e-6, 5.2e-6])
    frames.append(special[rng.integers(0, len(special), size=(H, W, 3))])
    mix = rng.uniform(0, 4, size=(H, W, 3))
    mix[rng.uniform(size=(H, W)) < 0.001] = on_boundary[7]  # a handful of flagged pixels: the per-pixel route
    frames.append(mix)
    sc = scenes.reflective_spheres()
    st = Settings(scenes.camera(W, H), sample_count=16, bounce_limit=4, seed=9)
    frames.append(oracle.OracleScene(sc).render_tiles(st.camera_settings, st, generate_tiles(W, H, (32, 32)), threads=4) / 16.0)
    fb = render.Framebuffer(gpu_ctx, W, H)
    for k, f in enumerate(frames):
        for spp, exposure, gamma in ((1, 1.0, 2.2), (16, 1.0, 2.2), (7, 0.5, 1.8)):
            acc = f * spp / exposure
            fb.upload(acc)
            got = render.resolve_tonemap(gpu_ctx, fb, spp, exposure, gamma)
            want = oracle.resolve_tonemap(acc, spp, exposure, gamma)
            assert np.array_equal(got, want), (k, spp, int((got != want).sum()))
    fb.close()


# ------------------------------------------------------------------ level 5: size-independent properties
def test_pass_splitting_and_accumulate_are_bit_exact(gpu_ctx):
    """One 12-sample launch == 5+7 samples in two launches (sample_begin) == += semantics on a pre-filled buffer."""
    sc = scenes.reflective_spheres()
    st = Settings(scenes.camera(200, 120), sample_count=12, bounce_limit=5, seed=77)
    cam = st.camera_settings
    tiles = generate_tiles(200, 120, (32, 32))  # ragged: 200 = 6*32 + 8, 120 = 3*32 + 24
    ds = render.DeviceScene(gpu_ctx, sc)
    fa, fb = render.Framebuffer(gpu_ctx, 200, 120), render.Framebuffer(gpu_ctx, 200, 120)
    render.render_tiles(gpu_ctx, ds, cam, st, tiles, fa, 0, 12)
    render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb, 0, 5)
    render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb, 5, 7)
    a, b = fa.download(), fb.download()
    assert a.tobytes() == b.tobytes()
    assert (a > 0).mean() > 0.3
    # zero-sample pass leaves the buffer untouched
    render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb, 12, 0)
    assert fb.download().tobytes() == a.tobytes()
    # accumulate on top of existing content
    base = np.random.default_rng(3).uniform(0, 1, a.shape)
    fb.upload(base)
    render.render_tiles(gpu_ctx, ds, cam, st, tiles[:5], fb, 0, 1)
    c = fb.download()
    untouched = np.ones((120, 200), dtype=bool)
    for (l, t, w, h) in tiles[:5]:
        untouched[t : t + h, l : l + w] = False
    assert (c[untouched] == base[untouched]).all()
    assert (c[~untouched] != base[~untouched]).any()
    fa.close(), fb.close(), ds.close()


def test_tile_shards_sum_to_the_full_image(gpu_ctx, small_mesh_scene):
    """8 disjoint round-robin tile shards rendered into zeroed buffers and summed == one full render, bit for bit
    (the multi-GPU reduce in miniature)."""
    st = Settings(scenes.camera(320, 180), sample_count=4, bounce_limit=5, seed=99)
    cam = st.camera_settings
    tiles = generate_tiles(320, 180, (32, 32))
    ds = render.DeviceScene(gpu_ctx, small_mesh_scene)
    full = render.Framebuffer(gpu_ctx, 320, 180)
    render.render_tiles(gpu_ctx, ds, cam, st, tiles, full)
    ref = full.download()
    total = np.zeros_like(ref)
    part = render.Framebuffer(gpu_ctx, 320, 180)
    for r in range(8):
        part.zero()
        render.render_tiles(gpu_ctx, ds, cam, st, tiles[r::8], part)
        total += part.download()
    assert total.tobytes() == ref.tobytes()
    full.close(), part.close(), ds.close()


def test_spheres_sum_inside_the_kernel_matches_the_direct_mode(gpu_ctx, oracle):
    """Split launches of the spheres kernel add a tile's samples inside the render kernel (the wave that finishes the tile last):
    whatever the split, over several passes of a capped scratch buffer, on ragged tiles and on top of previous contents, the frame
    is the one the direct mode (one wave per tile, the lane keeps its pixel's sum) and the oracle give, bit for bit."""
    sc = scenes.reflective_spheres()
    st = Settings(scenes.camera(203, 117), sample_count=40, bounce_limit=5, seed=77)  # 203 x 117: ragged wave tiles on both edges
    cam = st.camera_settings
    tiles = generate_tiles(203, 117, (32, 32))
    ds = render.DeviceScene(gpu_ctx, sc)
    fb = render.Framebuffer(gpu_ctx, 203, 117)
    base = np.random.default_rng(3).uniform(0, 1, (117, 203, 3))
    want = base + oracle.OracleScene(sc).render_tiles(cam, st, tiles, threads=4)
    out = {}
    bytes_per_sample = ((203 + 7) // 8) * ((117 + 7) // 8) * 64 * 32
    cap = max(1, (bytes_per_sample * 16) >> 20)
    # launch form 1 = one wave per work item, 2 = persistent workgroups (what full-size frames get)
    for split, cap_mb, mode in ((1, 0, 1), (1, 0, 2), (0, 0, 0), (2, 0, 1), (5, 0, 2), (10, 0, 1), (10, 0, 2), (5, cap, 1), (5, cap, 2)):
        gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, split), gpu_ctx.set_tunable(abi.RMD_TUNE_SCRATCH_CAP_MB, cap_mb)
        gpu_ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, mode)
        try:
            fb.upload(base)
            render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb)
            out[(split, cap_mb, mode)] = fb.download()
        finally:
            gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0), gpu_ctx.set_tunable(abi.RMD_TUNE_SCRATCH_CAP_MB, 0), gpu_ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 0)
    for key, img in out.items():
        assert img.tobytes() == out[(1, 0, 1)].tobytes(), key
    assert rel_close(out[(1, 0, 1)], want, 1e-9).mean() > 0.999
    fb.close(), ds.close()


def test_tile_rectangles_move_between_the_framebuffer_and_packed_host_buffers(gpu_ctx):
    """rmd_framebuffer_download_tiles / _upload_tiles (what a host scheduler uses to keep tile sums resident on the GPU and move only the tiles a
    message carries): every tile comes back as the same bits a whole-frame download holds there, in Tile.data layout, for ragged tiles, a subset in
    any order, and two downloads in flight; an upload changes exactly the tiles it names; rectangles outside the frame are refused."""
    import ctypes as C

    from raymond_amd.scene import tile_array

    W, H = 203, 117
    rng = np.random.default_rng(9)
    frame = rng.uniform(-1, 1, (H, W, 3))
    frame[5, 7] = [np.nan, np.inf, -0.0]
    fb = render.Framebuffer(gpu_ctx, W, H)
    fb.upload(frame)
    tiles = generate_tiles(W, H, (32, 32))
    order = list(rng.permutation(len(tiles)))
    some = [tiles[i] for i in order[: len(tiles) // 2]] + [(0, 0, 1, 1), (W - 3, H - 2, 3, 2), (0, 0, W, H)]
    for sel in (tiles, some):
        for (l, t, w, h), got in zip(sel, fb.download_tiles(sel)):
            assert same_bits(got, frame[t : t + h, l : l + w]).all(), (l, t, w, h)
    # two asynchronous downloads in flight, then a third (it waits for the first), into pinned memory
    L = gpu_ctx.L
    bufs = []
    for k in range(3):
        sel = tiles[k::3]
        n = sum(w * h for (_, _, w, h) in sel) * 3
        p = C.c_void_p()
        gpu_ctx.check(L.rmd_host_alloc(gpu_ctx.handle, n * 8, C.byref(p)))
        gpu_ctx.check(L.rmd_framebuffer_download_tiles_async(gpu_ctx.handle, fb.ptr, W, H, tile_array(sel), len(sel), p))
        bufs.append((sel, n, p))
    gpu_ctx.check(L.rmd_context_wait_transfers(gpu_ctx.handle))
    for sel, n, p in bufs:
        packed = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(n,)).copy()
        at = 0
        for (l, t, w, h) in sel:
            assert same_bits(packed[at : at + w * h * 3].reshape(h, w, 3), frame[t : t + h, l : l + w]).all()
            at += w * h * 3
        gpu_ctx.check(L.rmd_host_free(gpu_ctx.handle, p))
    # upload: only the named tiles change
    new = [rng.uniform(2, 3, (h, w, 3)) for (_, _, w, h) in tiles[::4]]
    fb.upload_tiles(tiles[::4], new)
    want = frame.copy()
    for (l, t, w, h), d in zip(tiles[::4], new):
        want[t : t + h, l : l + w] = d
    assert same_bits(fb.download(), want).all()
    bad = tile_array([(W - 8, 0, 16, 16)])
    out = np.zeros(16 * 16 * 3)
    assert L.rmd_framebuffer_download_tiles(gpu_ctx.handle, fb.ptr, W, H, bad, 1, out.ctypes.data_as(C.c_void_p)) == abi.RMD_ERR_INVALID_ARGUMENT
    fb.close()


def test_host_buffer_entry_point_matches_device_path(gpu_ctx):
    import ctypes as C

    sc = scenes.reflective_spheres()
    st = Settings(scenes.camera(64, 48), sample_count=3, bounce_limit=4, seed=5)
    cam = st.camera_settings
    tiles = generate_tiles(64, 48, (32, 32))
    ds = render.DeviceScene(gpu_ctx, sc)
    fb = render.Framebuffer(gpu_ctx, 64, 48)
    render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb)
    host = np.zeros((48, 64, 3))
    from raymond_amd.scene import tile_array

    c, s = cam.pod(), st.pod()
    gpu_ctx.check(gpu_ctx.L.rmd_render_tiles_host(gpu_ctx.handle, ds.handle, C.byref(c), C.byref(s), tile_array(tiles), len(tiles), host.ctypes.data_as(C.c_void_p)))
    assert host.tobytes() == fb.download().tobytes()
    fb.close(), ds.close()


def test_reference_shaped_api_end_to_end(gpu_ctx):
    """render_tiled(scene, settings).await_() — the reference's call sequence (cli_old/src/main.rs:152-153)."""
    sc = scenes.reflective_spheres()
    st = Settings(scenes.camera(96, 64), sample_count=8, tile_size=(32, 32), bounce_limit=5, seed=11)
    img = render.render_tiled(sc, st).await_()
    assert img.shape == (64, 96, 3) and np.isfinite(img).all()
    # progressive passes (samples_per_iteration, src/trace.rs:217-219) converge on the same sums
    st2 = Settings(scenes.camera(96, 64), sample_count=8, tile_size=(32, 32), bounce_limit=5, seed=11, samples_per_iteration=3)
    h = render.render_tiled(sc, st2)
    progressed = []
    h.set_callback(lambda tile: progressed.append(tile.sample_count))
    h.async_await()
    assert progressed and set(progressed) == {3, 6}
    assert h.await_().tobytes() == img.tobytes()
    # ceiling light: emission 1.5 seen directly by the top rows
    assert abs(img[0, 48].mean() - 1.5) < 1e-12


def test_error_paths(gpu_ctx):
    import ctypes as C

    from raymond_amd import abi, lib

    sc = scenes.reflective_spheres()
    ds = render.DeviceScene(gpu_ctx, sc)
    fb = render.Framebuffer(gpu_ctx, 32, 32)
    st = Settings(scenes.camera(32, 32), sample_count=1, bounce_limit=17)
    with pytest.raises(lib.RaymondError) as e:
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, [(0, 0, 32, 32)], fb)
    assert e.value.status == abi.RMD_ERR_UNSUPPORTED
    st = Settings(scenes.camera(32, 32), sample_count=1, bounce_limit=2)
    with pytest.raises(lib.RaymondError) as e:
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, [(16, 16, 32, 32)], fb)  # outside the backbuffer
    assert e.value.status == abi.RMD_ERR_INVALID_ARGUMENT
    assert b"outside" in gpu_ctx.L.rmd_last_error(gpu_ctx.handle)
    fb.close(), ds.close()
    # a roughness whose GGX angle could leave the device sin/cos' reduction range is refused at upload
    from raymond_amd.scene import Material, Object, Scene, Sphere

    wild = Scene()
    wild.objects.append(Object(Sphere((0.0, 0.0, 3.0), 1.0), Material.Metal((1.0, 1.0, 1.0), 1000.0)))
    with pytest.raises(lib.RaymondError) as e:
        render.DeviceScene(gpu_ctx, wild)
    assert e.value.status == abi.RMD_ERR_UNSUPPORTED


def test_sample_split_is_bit_exact(gpu_ctx, small_mesh_scene):
    """Launches with few wave tiles split each tile's sample range over K waves + an ordered summation kernel
    (api.cpp: choose_split).  Whatever K — forced, automatic, dividing the sample count or not — the frame must be
    bit-identical to the one-wave-per-tile launch, including += on a pre-filled buffer and ragged edge tiles."""
    import os

    st = Settings(scenes.camera(200, 120), sample_count=37, bounce_limit=5, seed=123)
    cam = st.camera_settings
    tiles = generate_tiles(200, 120, (32, 32))
    base = np.random.default_rng(5).uniform(0, 1, (120, 200, 3))
    for scene in (scenes.reflective_spheres(), small_mesh_scene):
        ds = render.DeviceScene(gpu_ctx, scene)
        fb = render.Framebuffer(gpu_ctx, 200, 120)
        results = {}
        for k in (1, 2, 4, 5, 0):  # 0 = automatic choice (this small frame splits)
            gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, k)
            try:
                fb.upload(base)
                render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb)
                results[k] = fb.download()
            finally:
                gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0)
        ref = results[1]
        assert (ref != base).any()
        for k, img in results.items():
            assert img.tobytes() == ref.tobytes(), "split %s differs" % k
        fb.close(), ds.close()


@pytest.mark.parametrize("dof,bounces,trace", [(False, 5, False), (True, 8, False), (False, 3, True), (True, 1, False)])
def test_role_sorted_trips_equal_the_lane_per_path_kernel(gpu_ctx, oracle, dof, bounces, trace):
    """The spheres kernel's split launches run trips sorted by role (render_kernel.hpp: render_wave_sorted — a wave's paths in an LDS pool, a trip
    is 64 new samples or 64 hits to shade); unsplit launches run the lane-per-path form.  Same frame bit for bit — ragged edge tiles
    (203 x 117), thin lens on and off, bounce limits 1 / 3 / 5 / 8, zero-throughput paths ended or traced, several sample splits incl. ones
    that do not divide the sample count, += on a pre-filled buffer — and equal to the oracle's."""
    W, H, spp = 203, 117, 29
    sc = scenes.reflective_spheres()
    st = Settings(scenes.camera(W, H, aperture_radius=0.5 if dof else 0.0), sample_count=spp, bounce_limit=bounces, seed=91, use_dof=dof, trace_black_paths=trace)
    cam = st.camera_settings
    tiles = generate_tiles(W, H, (32, 32))
    base = np.random.default_rng(8).uniform(0, 1, (H, W, 3))
    ds = render.DeviceScene(gpu_ctx, sc)
    fb = render.Framebuffer(gpu_ctx, W, H)
    frames = {}
    for k in (1, 2, 3, 7):
        gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, k)
        try:
            fb.upload(base)
            render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb)
            assert gpu_ctx.last_launch_info().split_k == k
            frames[k] = fb.download()
        finally:
            gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0)
    fb.close(), ds.close()
    for k in (2, 3, 7):
        assert frames[k].tobytes() == frames[1].tobytes(), "split %d (role-sorted trips) differs from the lane-per-path kernel" % k
    ref = oracle.OracleScene(sc).render_tiles(cam, st, tiles, accum=base.copy(), threads=4)
    ok = rel_close(frames[3], ref, 1e-9).all(axis=2)
    # (the accounting sums a pixel's samples from zero: the same launch into a zeroed buffer, and every pixel off in either comparison is handed over)
    from test_gpu_fullsize import account_for_off_pixels

    ds, fb = render.DeviceScene(gpu_ctx, sc), render.Framebuffer(gpu_ctx, W, H)
    gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 3)
    try:
        fb.zero()
        render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb)
        dev0 = fb.download()
    finally:
        gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0)
        fb.close(), ds.close()
    ref0 = oracle.OracleScene(sc).render_tiles(cam, st, tiles, threads=4)
    ok0 = rel_close(dev0, ref0, 1e-9).all(axis=2)
    account_for_off_pixels(gpu_ctx, oracle, sc, st, cam, spp, dev0, ref0, ok & ok0, "role-sorted trips dof=%s bounces=%d trace=%s" % (dof, bounces, trace))


@pytest.mark.parametrize("n_spheres", [61, 150, 900])
def test_role_sorted_trips_with_a_large_object_table(gpu_ctx, oracle, n_spheres):
    """(61 spheres: the room's planes are objects 61 .. 66 — the object loops take the turns of objects 0 .. 63 from a bit mask and visit the rest one
    by one, RenderParams::visit_mask.)  A scene of many objects leaves the persistent workgroups of the spheres kernel room for fewer LDS pools (150 spheres: 14 waves per
    workgroup; 900: none — the launch falls back to one wave per work item): same frame as the lane-per-path kernel bit for bit in every
    launch form, and the oracle's."""
    from raymond_amd.scene import Material, Object, Scene, Sphere

    rng = np.random.default_rng(n_spheres)
    sc = Scene()
    for i in range(n_spheres):
        c = (rng.uniform(-1.8, 1.8), rng.uniform(-0.9, 1.8), rng.uniform(1.5, 4.8))
        mat = Material.Metal(tuple(rng.uniform(0.2, 1.0, 3)), 0.05) if i % 3 == 0 else Material.Diffuse(tuple(rng.uniform(0.0, 1.0, 3)), 0.3)
        sc.objects.append(Object(Sphere(c, rng.uniform(0.03, 0.12)), mat))
    sc.objects.extend(scenes._room_planes())
    W, H, spp = 96, 64, 12
    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=4, seed=5)
    cam = st.camera_settings
    tiles = generate_tiles(W, H, (32, 32))
    ds = render.DeviceScene(gpu_ctx, sc)
    fb = render.Framebuffer(gpu_ctx, W, H)
    frames = {}
    for split, form in ((1, 0), (3, 0), (3, 2), (2, 1)):
        gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, split), gpu_ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, form)
        try:
            fb.zero()
            render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb)
            frames[(split, form)] = fb.download()
        finally:
            gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0), gpu_ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 0)
    fb.close(), ds.close()
    for key, img in frames.items():
        assert img.tobytes() == frames[(1, 0)].tobytes(), key
    ref = oracle.OracleScene(sc).render_tiles(cam, st, tiles, threads=4)
    from test_gpu_fullsize import account_for_off_pixels

    ok = rel_close(frames[(3, 2)], ref, 1e-9).all(axis=2)
    account_for_off_pixels(gpu_ctx, oracle, sc, st, cam, spp, frames[(3, 2)], ref, ok, "role-sorted trips, %d spheres" % n_spheres)


def test_object_turns_past_the_masks_reach(gpu_ctx, oracle):
    """The object loops take the turns of objects 0 .. 63 from bit masks made at scene creation (RenderParams::visit_mask / grid_mask: the planes the
    axis rule has dealt with are passed by, intersect_grids visits grids only) and visit objects from 64 on one by one.  A mesh scene with 70
    spheres in FRONT of its room and its mesh (the paired planes and the grid are objects 70 .. 77) and one with 60 (the room straddles 64): the
    queued and the lane-per-path kernel give the same frame bit for bit, and the oracle's."""
    from raymond_amd.scene import Material, Object, Sphere

    for n_front in (70, 60):
        rng = np.random.default_rng(n_front)
        sc = scenes.mesh_scene(scenes.lumpy_sphere_mesh(11))
        front = []
        for i in range(n_front):
            c = (rng.uniform(-1.8, 1.8), rng.uniform(-0.9, 1.8), rng.uniform(1.5, 4.8))
            mat = Material.Metal(tuple(rng.uniform(0.2, 1.0, 3)), 0.05) if i % 3 == 0 else Material.Diffuse(tuple(rng.uniform(0.0, 1.0, 3)), 0.3)
            front.append(Object(Sphere(c, rng.uniform(0.03, 0.1)), mat))
        sc.objects[:0] = front
        W, H, spp = 96, 64, 16
        st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=4, seed=9)
        cam = st.camera_settings
        tiles = generate_tiles(W, H, (32, 32))
        ds, fb = render.DeviceScene(gpu_ctx, sc), render.Framebuffer(gpu_ctx, W, H)
        frames = {}
        for queues, split in ((0, 4), (1, 4), (1, 1)):
            gpu_ctx.set_tunable(abi.RMD_TUNE_PATH_QUEUES, queues), gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, split)
            gpu_ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 2 if split > 1 else 0)  # (2: persistent workgroups although the frame has few work items)
            try:
                fb.zero()
                render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb)
                frames[(queues, split)] = fb.download()
                if (queues, split) == (0, 4):
                    assert gpu_ctx.last_launch_info().queued == 1
            finally:
                gpu_ctx.set_tunable(abi.RMD_TUNE_PATH_QUEUES, 0), gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0), gpu_ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 0)
        fb.close(), ds.close()
        for key, img in frames.items():
            assert same_bits(img, frames[(0, 4)]).all(), (n_front, key)
        ref = oracle.OracleScene(sc).render_tiles(cam, st, tiles, threads=8)
        assert rel_close(frames[(0, 4)], ref, 1e-9).all(axis=2).mean() >= 0.995, n_front


def test_walks_put_aside_do_not_change_the_image(gpu_ctx, small_mesh_scene):
    """Grid scenes: a walk call of a wave stops stepping under its last K rays and leaves their walks — DDA state stored — to the wave's next
    call (grid_walk.hpp: WalkCarry; RMD_TUNE_WALK_CUT = K + 1).  Every ray takes the same steps and the same tests in the same order whenever it
    takes them, so every K, with every batch size, in both launch forms, must give the frame of K = 0 (every call finishes every walk)."""
    st = Settings(scenes.camera(192, 128), sample_count=24, bounce_limit=5, seed=78)
    cam = st.camera_settings
    tiles = generate_tiles(192, 128, (32, 32))
    ds = render.DeviceScene(gpu_ctx, small_mesh_scene)
    fb = render.Framebuffer(gpu_ctx, 192, 128)
    frames = {}
    try:
        for split, batch, cut in [(1, 0, 1), (1, 0, 0), (1, 0, 3), (1, 0, 9), (1, 0, 32), (3, 0, 1), (3, 0, 0), (3, 0, 2), (3, 0, 5), (3, 0, 17), (3, 16, 7), (3, 64, 13), (0, 0, 0)]:
            gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, split), gpu_ctx.set_tunable(abi.RMD_TUNE_WALK_BATCH, batch), gpu_ctx.set_tunable(abi.RMD_TUNE_WALK_CUT, cut)
            fb.zero()
            render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb)
            frames[(split, batch, cut)] = fb.download().tobytes()
    finally:
        gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0), gpu_ctx.set_tunable(abi.RMD_TUNE_WALK_BATCH, 0), gpu_ctx.set_tunable(abi.RMD_TUNE_WALK_CUT, 0)
    assert len(set(frames.values())) == 1
    fb.close(), ds.close()


def test_chained_work_items_do_not_change_the_image(gpu_ctx, small_mesh_scene, oracle):
    """Short split launches of scenes with grids run the instantiation whose persistent waves draw their next work item while the last paths of
    the current one finish (render_kernel.hpp: render_wave, CHAIN; a path's pixel, sample and scratch sector live per lane).  Which lane, trip and
    wave compute a sample changes nothing: chained, unchained and direct launches give the same frame bit for bit — ragged tiles, thin lens,
    several passes of the scratch, any split — and the oracle's."""
    W, H = 203, 117
    tiles = generate_tiles(W, H, (32, 32))
    ds = render.DeviceScene(gpu_ctx, small_mesh_scene)
    fb = render.Framebuffer(gpu_ctx, W, H)
    for spp, dof, bounces in ((12, False, 5), (40, True, 8), (3, False, 2)):
        st = Settings(scenes.camera(W, H, aperture_radius=0.4 if dof else 0.0), sample_count=spp, bounce_limit=bounces, seed=77, use_dof=dof)
        frames = {}
        for name, chain, split, cap in (("chained", 2, 0, 0), ("unchained", 1, 0, 0), ("chained-many-items", 2, 5, 0), ("chained-two-passes", 2, 0, 1), ("direct", 1, 1, 0)):
            gpu_ctx.set_tunable(abi.RMD_TUNE_CHAIN_ITEMS, chain), gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, split)
            gpu_ctx.set_tunable(abi.RMD_TUNE_SCRATCH_CAP_MB, cap), gpu_ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 2)
            gpu_ctx.set_tunable(abi.RMD_TUNE_PATH_QUEUES, 1)  # the lane-per-path form (the queued form: test_path_queues_do_not_change_the_image)
            try:
                fb.zero()
                render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb)
                info = gpu_ctx.last_launch_info()
                frames[name] = fb.download()
                if name == "chained-many-items" and spp < 8:
                    assert info.buffered == 0  # (a forced split keeps 4 samples per item: 3 samples run in direct mode)
                elif name.startswith("chained"):
                    assert info.chained == 1 and info.persistent == 1 and info.buffered == 1, (name, info.chained, info.persistent)
                else:
                    assert info.chained == 0
                if name == "chained-two-passes" and spp >= 16:
                    assert info.passes >= 2
            finally:
                for key in (abi.RMD_TUNE_CHAIN_ITEMS, abi.RMD_TUNE_SAMPLE_SPLIT, abi.RMD_TUNE_SCRATCH_CAP_MB, abi.RMD_TUNE_LAUNCH_FORM, abi.RMD_TUNE_PATH_QUEUES):
                    gpu_ctx.set_tunable(key, 0)
        for name, img in frames.items():
            assert same_bits(img, frames["direct"]).all(), (spp, name)
        ref = oracle.OracleScene(small_mesh_scene).render_tiles(st.camera_settings, st, tiles, threads=8)
        from test_gpu_fullsize import account_for_off_pixels

        ok = rel_close(frames["chained"], ref, 1e-9).all(axis=2)
        account_for_off_pixels(gpu_ctx, oracle, small_mesh_scene, st, st.camera_settings, spp, frames["chained"], ref, ok, "chained work items spp=%d dof=%s bounces=%d" % (spp, dof, bounces))
    fb.close(), ds.close()


def test_path_queues_do_not_change_the_image(gpu_ctx, small_mesh_scene, oracle):
    """Persistent split launches of scenes with grids keep their paths in per-wave queues in device memory (render_kernel.hpp: render_wave_queued —
    ray compaction between bounces: a trip is 64 new samples, 64 parked hits or one grid walk for 64 parked rays; hits are held in their lanes when
    the next trip shades them anyway; walks that are put aside go back onto the ray stack with their DDA state).  Which lane, trip and wave compute
    a sample changes nothing: the queued form, the lane-per-path forms and the direct launch give the same frame bit for bit — ragged tiles, thin
    lens, black paths ended or traced, several passes of the scratch, any split, walks put aside or not, one grid or two — and the oracle's."""
    from raymond_amd.scene import AccGrid, Grid, Material, Object, Plane, Scene

    two = Scene()  # two grid objects: no walk is put aside there (the carried state is one walk's), every WALK trip walks both grids
    two.objects.append(Object(Grid(AccGrid.build_from_mesh(scenes.lumpy_sphere_mesh(6, (0.9, 0.9, 0.5), (-0.6, -0.2, 2.6)))), Material.Metal((1.0, 1.0, 0.1), 0.15)))
    two.objects.append(Object(Plane((0.0, -1.0, 0.0), (0.0, 1.0, 0.0)), Material.Diffuse((0.75, 0.75, 0.75), 0.5)))
    two.objects.append(Object(Grid(AccGrid.build_from_mesh(scenes.lumpy_sphere_mesh(5, (1.0, 1.1, 0.7), (0.5, 0.0, 2.9)))), Material.Diffuse((0.2, 0.8, 0.3), 0.4)))
    two.objects.append(Object(Plane((0.0, 2.0, 0.0), (0.0, -1.0, 0.0)), Material.Emission((1.5, 1.5, 1.5))))
    W, H = 203, 117
    tiles = generate_tiles(W, H, (32, 32))
    T = abi
    keys = (T.RMD_TUNE_PATH_QUEUES, T.RMD_TUNE_SAMPLE_SPLIT, T.RMD_TUNE_SCRATCH_CAP_MB, T.RMD_TUNE_LAUNCH_FORM, T.RMD_TUNE_WALK_CUT, T.RMD_TUNE_CHAIN_ITEMS)
    for sc, spp, dof, bounces, end_black, mask_budget in ((small_mesh_scene, 12, False, 5, False, 0), (small_mesh_scene, 40, True, 8, False, 0), (small_mesh_scene, 24, False, 5, True, 0),
                                                          (small_mesh_scene, 3, False, 2, False, 0), (small_mesh_scene, 1, False, 5, False, 0), (two, 16, False, 5, False, 0),
                                                          (small_mesh_scene, 16, False, 5, False, 256)):  # (256 bytes of mask: one bit covers several cells — the walk's general stepping loop)
        gpu_ctx.set_tunable(T.RMD_TUNE_MASK_BUDGET, mask_budget)
        try:
            ds = render.DeviceScene(gpu_ctx, sc)
        finally:
            gpu_ctx.set_tunable(T.RMD_TUNE_MASK_BUDGET, 0)
        fb = render.Framebuffer(gpu_ctx, W, H)
        st = Settings(scenes.camera(W, H, aperture_radius=0.4 if dof else 0.0), sample_count=spp, bounce_limit=bounces, seed=77, use_dof=dof, end_black_paths=end_black)
        frames = {}
        #            name                 queues split cap form cut
        variants = (("queued",               0,    0,   0,   2,  0),
                    ("queued-many-items",    0,    5,   0,   2,  0),
                    ("queued-two-passes",    0,    0,   1,   2,  0),
                    ("queued-no-walk-cut",   0,    0,   0,   2,  1),
                    ("queued-cut-of-12",     0,    0,   0,   2, 13),
                    ("lane-per-path",        1,    0,   0,   2,  0),
                    ("one-wave-per-item",    0,    3,   0,   1,  0),
                    ("direct",               1,    1,   0,   0,  0))
        for name, queues, split, cap, form, cut in variants:
            for key, val in zip(keys, (queues, split, cap, form, cut, 0)):
                gpu_ctx.set_tunable(key, val)
            try:
                fb.zero()
                render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb)
                info = gpu_ctx.last_launch_info()
                frames[name] = fb.download()
                if name.startswith("queued") and not (name == "queued-many-items" and spp < 8):
                    assert info.queued == 1 and info.persistent == 1 and info.buffered == 1 and info.chained == 0, (name, spp, info.queued, info.persistent, info.buffered)
                else:
                    assert info.queued == 0, name
                if name == "queued-two-passes" and spp >= 16:
                    assert info.passes >= 2
            finally:
                for key in keys:
                    gpu_ctx.set_tunable(key, 0)
        for name, img in frames.items():
            assert same_bits(img, frames["direct"]).all(), (spp, dof, end_black, name)
        ref = oracle.OracleScene(sc).render_tiles(st.camera_settings, st, tiles, threads=8)
        if not end_black:  # (the oracle traces every path: flags 0)
            from test_gpu_fullsize import account_for_off_pixels

            ok = rel_close(frames["queued"], ref, 1e-9).all(axis=2)
            account_for_off_pixels(gpu_ctx, oracle, sc, st, st.camera_settings, spp, frames["queued"], ref, ok,
                                   "path queues %s spp=%d dof=%s bounces=%d mask budget %d" % ("two grids" if sc is two else "one grid", spp, dof, bounces, mask_budget))
        fb.close(), ds.close()


def test_walk_batching_does_not_change_the_image(gpu_ctx, small_mesh_scene):
    """Grid scenes: a lane whose ray enters a grid's box waits until enough lanes of its wave need a walk (kernels.hip,
    RenderParams::walk_batch).  That is scheduling only — the closest hit is the lexicographic minimum of (distance,
    object index) whatever the order — so every batch size must give the same frame, with one wave per tile (lane =
    pixel) and with split sample ranges (lanes draw (pixel, sample) items from a pool) alike."""
    import os

    st = Settings(scenes.camera(160, 96), sample_count=24, bounce_limit=5, seed=77)
    cam = st.camera_settings
    tiles = generate_tiles(160, 96, (32, 32))
    ds = render.DeviceScene(gpu_ctx, small_mesh_scene)
    fb = render.Framebuffer(gpu_ctx, 160, 96)
    frames = {}
    try:
        for split in (1, 3):
            for batch in (1, 7, 32, 64, 1000):
                gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, split), gpu_ctx.set_tunable(abi.RMD_TUNE_WALK_BATCH, batch)
                fb.zero()
                render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb)
                frames[(split, batch)] = fb.download().tobytes()
    finally:
        gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0), gpu_ctx.set_tunable(abi.RMD_TUNE_WALK_BATCH, 0)
    assert len(set(frames.values())) == 1
    fb.close(), ds.close()


def test_degenerate_scenes_and_frames(gpu_ctx, oracle):
    """Empty scene (every ray misses), 1x1 frame, a single 3x5 tile off the 8-pixel lattice."""
    from raymond_amd.scene import Scene

    empty = Scene()
    st = Settings(scenes.camera(40, 24), sample_count=3, bounce_limit=5, seed=1)
    ds = render.DeviceScene(gpu_ctx, empty)
    fb = render.Framebuffer(gpu_ctx, 40, 24)
    render.render_tiles(gpu_ctx, ds, st.camera_settings, st, generate_tiles(40, 24, (32, 32)), fb)
    assert not fb.download().any()
    fb.close(), ds.close()
    sc = scenes.reflective_spheres()
    osc = oracle.OracleScene(sc)
    for (w, h, tiles) in ((1, 1, [(0, 0, 1, 1)]), (37, 29, [(5, 3, 3, 5), (20, 11, 17, 18)])):
        st = Settings(scenes.camera(w, h), sample_count=6, bounce_limit=4, seed=17)
        ds = render.DeviceScene(gpu_ctx, sc)
        fb = render.Framebuffer(gpu_ctx, w, h)
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb)
        dev = fb.download()
        ref = osc.render_tiles(st.camera_settings, st, tiles)
        from test_gpu_fullsize import account_for_off_pixels

        ok = rel_close(dev, ref, 1e-9).all(axis=2)
        account_for_off_pixels(gpu_ctx, oracle, sc, st, st.camera_settings, 6, dev, ref, ok, "degenerate frame %dx%d" % (w, h))
        covered = np.zeros((h, w), dtype=bool)
        for (l, t, tw, th) in tiles:
            covered[t : t + th, l : l + tw] = True
        assert not dev[~covered].any()
        fb.close(), ds.close()


def test_two_grids_and_coarse_masks(gpu_ctx, oracle):
    """A scene with two AccGrids (two occupancy masks in LDS, objects interleaved with planes), rendered with the
    exact masks and with a mask budget so small that one bit covers many cells (false-positive candidates)."""
    import os

    from raymond_amd.scene import AccGrid, Grid, Material, Object, Plane, Scene, Sphere

    def mesh(n, centre, extent):
        m = scenes.lumpy_sphere_mesh(n, extent=extent, centre=centre)
        m.bake_transform((0.0, -0.3, 2.9))
        return m

    sc = Scene()
    sc.objects.append(Object(Grid(AccGrid.build_from_mesh(mesh(14, (-0.9, 0.0, 0.0), (1.2, 1.0, 0.8)))), Material.Metal((1.0, 1.0, 0.1), 0.15)))
    sc.objects.append(Object(Plane((0.0, -1.0, 0.0), (0.0, 1.0, 0.0)), Material.Diffuse((0.75, 0.75, 0.75), 0.5)))
    sc.objects.append(Object(Grid(AccGrid.build_from_mesh(mesh(10, (0.9, 0.1, 0.3), (1.0, 1.1, 0.7)))), Material.Diffuse((0.2, 0.8, 0.3), 0.4)))
    sc.objects.append(Object(Plane((0.0, 2.0, 0.0), (0.0, -1.0, 0.0)), Material.Emission((1.5, 1.5, 1.5))))
    sc.objects.append(Object(Sphere((0.0, -0.6, 2.2), 0.3), Material.Diffuse((1.0, 0.0, 0.0), 0.02)))
    st = Settings(scenes.camera(320, 180), sample_count=1, bounce_limit=5, seed=77)
    cam = st.camera_settings
    rng = np.random.default_rng(3)
    n = 12000
    xy = np.stack([rng.integers(0, 320, n), rng.integers(0, 180, n)], axis=1).astype(np.uint32)
    smp = rng.integers(0, 1000, n).astype(np.uint32)
    osc = oracle.OracleScene(sc)
    orgb = osc.trace_samples(cam, st, xy, smp)
    for budget in (None, 256):
        gpu_ctx.set_tunable(abi.RMD_TUNE_MASK_BUDGET, budget or 0)
        try:
            ds = render.DeviceScene(gpu_ctx, sc)
        finally:
            gpu_ctx.set_tunable(abi.RMD_TUNE_MASK_BUDGET, 0)
        drgb, dpo, dps = probe.trace_samples(gpu_ctx, ds, cam, st, xy, smp, paths=True)
        close = rel_close(drgb, orgb, 1e-9).all(axis=1)
        assert close.mean() >= 0.999, (budget, close.mean())
        assert (dpo == 0).any(axis=1).mean() > 0.02 and (dpo == 2).any(axis=1).mean() > 0.02  # both meshes are hit
        # a full-frame launch takes the same path (tile mode, sample splitting on)
        fb = render.Framebuffer(gpu_ctx, 320, 180)
        render.render_tiles(gpu_ctx, ds, cam, st, generate_tiles(320, 180, (32, 32)), fb)
        img = fb.download()
        assert np.isfinite(img).all()
        if budget is None:
            exact = img
        else:
            assert img.tobytes() == exact.tobytes()  # the mask only filters: coarse or exact, same image
        fb.close(), ds.close()


def test_launch_forms_of_grid_scenes_are_bit_identical(gpu_ctx, small_mesh_scene, oracle):
    """The mesh kernel's launch forms — persistent workgroups drawing work items from a counter, one wave per work item — direct and
    split: same arithmetic, same per-sample output => the same frame bit for bit: thin lens, += on a pre-filled buffer, ragged tiles,
    a sub-range of samples, bounce limits 0, 1 and 8, and a scene with two grids."""
    from raymond_amd.scene import AccGrid, Grid, Material, Object, Plane, Scene, Sphere

    two = Scene()
    two.objects.append(Object(Grid(AccGrid.build_from_mesh(scenes.lumpy_sphere_mesh(6, (0.9, 0.9, 0.5), (-0.6, -0.2, 2.6)))), Material.Metal((1.0, 1.0, 0.1), 0.15)))
    two.objects.append(Object(Plane((0.0, -1.0, 0.0), (0.0, 1.0, 0.0)), Material.Diffuse((0.75, 0.75, 0.75), 0.5)))
    two.objects.append(Object(Grid(AccGrid.build_from_mesh(scenes.lumpy_sphere_mesh(5, (1.0, 1.1, 0.7), (0.5, 0.0, 2.9)))), Material.Diffuse((0.2, 0.8, 0.3), 0.4)))
    two.objects.append(Object(Plane((0.0, 2.0, 0.0), (0.0, -1.0, 0.0)), Material.Emission((1.5, 1.5, 1.5))))
    cases = [
        (small_mesh_scene, Settings(scenes.camera(200, 120), sample_count=9, bounce_limit=5, seed=5), 0, 9),
        (small_mesh_scene, Settings(scenes.camera(200, 120, aperture_radius=0.5), sample_count=12, bounce_limit=8, seed=6, use_dof=True), 3, 9),
        (small_mesh_scene, Settings(scenes.camera(64, 40), sample_count=8, bounce_limit=1, seed=8), 0, 8),
        (small_mesh_scene, Settings(scenes.camera(64, 40), sample_count=4, bounce_limit=0, seed=7), 0, 4),
        (two, Settings(scenes.camera(160, 96), sample_count=8, bounce_limit=5, seed=9), 0, 8),
    ]
    for sc, st, begin, count in cases:
        cam = st.camera_settings
        W, H = cam.backbuffer_width, cam.backbuffer_height
        tiles = generate_tiles(W, H, (32, 32))
        base = np.random.default_rng(1).uniform(0, 1, (H, W, 3))
        ds = render.DeviceScene(gpu_ctx, sc)
        fb = render.Framebuffer(gpu_ctx, W, H)
        out = {}
        # form 0 = the library's choice (one wave per work item for frames this small), 2 = persistent workgroups drawing work items
        # from a counter (what full-size frames get), 1 = one wave per work item;
        # (form, forced split): 0 = the library's choice (direct mode for these few samples), 3 = three waves per wave tile
        for mode, split in ((0, 0), (1, 0), (2, 0), (0, 3), (1, 3), (2, 3)):
            gpu_ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, mode)
            gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, split)
            try:
                fb.upload(base)
                render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb, begin, count)
                out[(mode, split)] = fb.download()
            finally:
                gpu_ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 0), gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0)
        for key, img in out.items():
            assert img.tobytes() == out[(0, 0)].tobytes(), (W, H, key)
        if st.bounce_limit:
            assert (out[(0, 0)] != base).any()
        fb.close(), ds.close()


# ------------------------------------------------------------------ the HIP path against the SECOND reading of the reference source
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["spheres", "mesh", "mesh-thin-lens"])
def test_per_sample_against_the_second_reading_of_the_source(gpu_ctx, small_mesh_scene, what):
    """tests/second_reading.py restates the whole path a second time, in plain Python floats, from the Rust text alone (it shares no code with
    oracle/oracle.cpp; tests/test_second_reading.py holds the oracle against it bit for bit).  Here the HIP kernel itself is held against it,
    sample by sample — vertex sequence (object and triangle at every depth) and radiance to the stated 1e-9 — without the C++ oracle in between."""
    import second_reading as sr
    from test_second_reading import second_reading_scene

    if what == "spheres":
        scene, st, n = scenes.reflective_spheres(), scenes.config_settings("C2"), 20000
    else:
        lens = what == "mesh-thin-lens"
        scene = small_mesh_scene
        st = Settings(scenes.camera(480, 270, aperture_radius=0.5 if lens else 0.0), sample_count=1, bounce_limit=5, seed=scenes.SEED + 11, use_dof=lens)
        n = 12000
    cam = st.camera_settings
    rng = np.random.default_rng(41)
    xy = np.stack([rng.integers(0, cam.backbuffer_width, n), rng.integers(0, cam.backbuffer_height, n)], axis=1).astype(np.uint32)
    smp = rng.integers(0, 4000, n).astype(np.uint32)
    ds = render.DeviceScene(gpu_ctx, scene)
    drgb, dpo, dps = probe.trace_samples(gpu_ctx, ds, cam, st, xy, smp, paths=True)
    ds.close()
    sc, c = second_reading_scene(scene, cam)
    same_path, close, lit, through_mesh = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), 0, 0
    for i in range(n):
        path = []
        rgb = sr.sample_pixel(sc, c, {"bounce_limit": st.bounce_limit}, st.seed, int(xy[i, 0]), int(xy[i, 1]), int(smp[i]), use_dof=st.use_dof, path=path)
        k = len(path)
        same_path[i] = dpo[i, :k].tolist() == [p[0] for p in path] and dps[i, :k].tolist() == [p[1] for p in path] and (dpo[i, k:] == -2).all()
        close[i] = rel_close(drgb[i], np.asarray(rgb), 1e-9).all()
        lit += any(v != 0.0 for v in rgb)
        through_mesh += any(p[0] == 1 for p in path)
    assert close[same_path].all(), "a sample with the second reading's exact vertex sequence differs beyond 1e-9"
    assert same_path.mean() >= 0.999 and close.mean() >= 0.999
    assert lit > n // 20 and (what == "spheres" or through_mesh > n // 20)
