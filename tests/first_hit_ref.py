"""The expected sums of rmd_render_features, composed from the oracle's entry points and nothing else:
orc_sample_primary_rays (the sample's own stream: the pixel jitter, then the thin lens' rounds where use_dof asks for them) -> orc_scene_intersect
-> the plane's stored normal / orc_sphere_normal / orc_triangle_normal, the material's colour and t; sequential sums in sample order.  A sample the
thin lens yields no ray for (ok == 0) is seven zeros, like a miss.  tests/test_first_hit_host.py holds this composition to the oracle's render path
(orc_trace_sample's first vertex), to the former pinhole composition (orc_block_uniforms -> orc_primary_ray, kept below as pinhole_rays) and to
the second reading of the source."""
import collections
import ctypes as C
import functools

import numpy as np

import oracle_lib as O

GROUPS = (slice(0, 3), slice(3, 6), slice(6, 7))  # normal, albedo, depth


def pixel_grid(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.ascontiguousarray(np.stack([xs.ravel(), ys.ravel()], 1).astype(np.uint32))
    return xy, (ys * W + xs).ravel()


def hit_features(scene, rays, obj, t, sub):
    """(n, 7) feature vectors of the hits (obj, t, sub) of `rays` (obj < 0: a miss, seven zeros)."""
    L = O.load()
    objs, _, descs, _, _keep = scene.flatten()
    f = np.zeros((len(obj), 7))
    for i in np.unique(obj):
        if i < 0:
            continue
        m = obj == i
        k = int(m.sum())
        o = objs[i]
        f[m, 3:6] = list(o.material.color)
        f[m, 6] = t[m]
        R, T = np.ascontiguousarray(rays[m]), np.ascontiguousarray(t[m])
        n3 = np.zeros((k, 3))
        if o.geometry_kind == 0:
            n3[:] = list(o.normal)
        elif o.geometry_kind == 1:
            sp = np.ascontiguousarray(np.tile(np.array(list(o.origin) + [o.radius]), (k, 1)))
            L.orc_sphere_normal(k, O.ptr(sp), O.ptr(R), O.ptr(T), O.ptr(n3))
        else:
            g = descs[o.grid_index]
            tp = np.ctypeslib.as_array(C.cast(g.tri_pos, C.POINTER(C.c_double)), (g.n_tris, 9))
            tn = np.ctypeslib.as_array(C.cast(g.tri_nrm, C.POINTER(C.c_double)), (g.n_tris, 9))
            L.orc_triangle_normal(k, O.ptr(np.ascontiguousarray(tp[sub[m]])), O.ptr(np.ascontiguousarray(tn[sub[m]])), O.ptr(R), O.ptr(T), O.ptr(n3))
        f[m, 0:3] = n3
    return f


def pinhole_rays(cam, seed, xy, pix, sample):
    """the pinhole rays of one sample index by the composition this module used before the oracle had orc_sample_primary_rays"""
    u = np.ascontiguousarray(O.block_uniforms(seed, pix, [sample] * len(pix), [0] * len(pix))[:, :2])
    rays = np.zeros((len(pix), 6))
    c = cam.pod()
    O.load().orc_primary_ray(len(pix), C.byref(c), O.ptr(np.ascontiguousarray(xy, dtype=np.uint32)), O.ptr(u), O.ptr(rays))
    return rays


def sample_features(scene, osc, cam, seed, use_dof, xy, samples):
    """-> phi (n, 7), obj (n,), t (n,), sub (n,), ok (n,), rays (n, 6) of the (x, y, sample) triples; obj == -1: a miss or no ray"""
    rays, ok = O.sample_primary_rays(cam, seed, use_dof, xy, samples)
    obj, t, sub = osc.scene_intersect(rays)
    obj = np.where(ok != 0, obj, -1).astype(np.int32)  # (a ray of six zeros hits nothing anyway: NaN distances everywhere)
    return hit_features(scene, rays, obj, t, sub), obj, t, sub, ok, rays


def group_max(a):
    """(..., 7) -> (..., 3): the largest value of each group (normal, albedo, depth), a NaN counting as 0"""
    a = np.where(np.isnan(a), 0.0, a)
    return np.stack([a[..., g].max(axis=-1) for g in GROUPS], axis=-1)


def first_hit_sums(scene, cam, seed, spp, sample_begin=0, use_dof=False, scales=False):
    """-> F, G (H, W, 7): the sums and sums of squares of the first-hit features of samples sample_begin .. + spp - 1, and the per-sample object
    indices (spp, H, W), -1 for a miss and for a sample without a ray.  scales=True: also TF, TG (H, W, 3), the term scales per pixel and group
    (normal, albedo, depth): T = sum over the samples of max over the group's channels of |phi| (for G: of phi^2) — what outside_the_pixel_bar
    measures a difference by — and the per-sample distances (spp, H, W), NaN where there is no hit."""
    W, H = cam.backbuffer_width, cam.backbuffer_height
    osc = O.OracleScene(scene)
    xy, pix = pixel_grid(W, H)
    F, G = np.zeros((H, W, 7)), np.zeros((H, W, 7))
    TF, TG = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    objs, ts = [], []
    for s in range(sample_begin, sample_begin + spp):
        f, obj, t = sample_features(scene, osc, cam, seed, use_dof, xy, np.full(len(pix), s, dtype=np.uint32))[:3]
        f = f.reshape(H, W, 7)
        F = F + f
        G = G + f * f
        TF = TF + group_max(np.abs(f))
        TG = TG + group_max(f * f)
        objs.append(obj.reshape(H, W).copy())
        ts.append(np.where(obj >= 0, t, np.nan).reshape(H, W))
    return (F, G, np.stack(objs), TF, TG, np.stack(ts)) if scales else (F, G, np.stack(objs))


def outside_the_bar(dev, ref):
    """Values with |dev - ref| > 1e-9 * max(|ref|, m), m the frame's largest |ref| in the value's group (normal, albedo or depth); a NaN only
    matches a NaN.  -> boolean array of dev's shape."""
    bad = np.zeros(ref.shape, dtype=bool)
    for g in GROUPS:
        r, d = ref[..., g], dev[..., g]
        fin = np.isfinite(r)
        m = np.abs(r[fin]).max() if fin.any() else 0.0
        with np.errstate(all="ignore"):
            ok = np.abs(d - r) <= 1e-9 * np.maximum(np.abs(r), m)
        ok = np.where(np.isnan(r), np.isnan(d), ok)
        bad[..., g] = ~ok
    return bad


def outside_the_pixel_bar(dev, ref, T):
    """Values with |dev - ref| > 1e-9 * T, T (H, W, 3) the term scale of the value's pixel and group (first_hit_sums(scales=True)); a NaN only
    matches a NaN.  1e-9 is the project's bar; T bounds what rounding a sum of those terms can do (a sequential f64 sum of n terms is within
    n * 2^-53 * sum |term| of the exact one, and each term within a few 2^-53 of its own size).  Where T is 0 — every sample at t = 0, or every
    sample a miss — the values must be equal.  -> boolean array of dev's shape."""
    bad = np.zeros(ref.shape, dtype=bool)
    for k, g in enumerate(GROUPS):
        r, d = ref[..., g], dev[..., g]
        with np.errstate(all="ignore"):
            ok = np.abs(d - r) <= 1e-9 * T[..., k : k + 1]
        ok = np.where(np.isnan(r), np.isnan(d), ok)
        bad[..., g] = ~ok
    return bad


def worst_over_scale(dev, ref, T):
    """-> [largest |dev - ref| / T per group] over the values whose reference is finite and whose T is not 0 (0.0 where there is none)"""
    out = []
    for k, g in enumerate(GROUPS):
        with np.errstate(all="ignore"):
            q = np.abs(dev[..., g] - ref[..., g]) / T[..., k : k + 1]
        q = q[np.isfinite(ref[..., g]) & np.isfinite(q)]
        out.append(float(q.max()) if q.size else 0.0)
    return out


# ---------------------------------------------------------------- the adversarial scenes as feature cases (tests/sphere_scenes.py, tests/mesh_scenes.py)
# A key is (kind, class, seed, lens, edge): kind "spheres" or "mesh", edge None or a label of LENS_EDGES.  The frames are the classes' own; 6 samples
# instead of the classes' 160 or 48 (the kernel's sample loop carries no state beyond the sums), from sample 5 on odd seeds.
FEATURE_SPP = 6
EDGE_FRAME = (40, 24)
EDGE_BASES = (("spheres", "shuffled_room", 1, False), ("mesh", "shared_grid", 0, False))
# label -> (focal_length, aperture_radius); every one is rendered with use_dof
LENS_EDGES = {"focal-negative": (-2.5, 0.5), "focal-zero": (0.0, 0.5), "focal-1e-3": (1e-3, 0.5), "focal-1e6": (1e6, 0.5), "aperture-1e-9": (2.5, 1e-9),
              "aperture-4": (2.5, 4.0), "aperture-zero": (2.5, 0.0), "focal-nan": (float("nan"), 0.5)}
EDGE_EXTRA = (("mesh", "open_scene", 0, False, "aperture-4"),)  # in a closed room no lens ray misses; over a scene without walls some do
FeatureCase = collections.namedtuple("FeatureCase", "key scene cam settings seed use_dof begin spp tunables")
Reference = collections.namedtuple("Reference", "F G objs TF TG t")


def feature_keys(lens_edges=False):
    import mesh_scenes as ms
    import sphere_scenes as ss

    if lens_edges:
        return [base + (label,) for base in EDGE_BASES for label in LENS_EDGES] + list(EDGE_EXTRA)
    return [("spheres",) + tuple(c) + (None,) for c in ss.cases()] + [("mesh",) + tuple(c) + (None,) for c in ms.cases()]


def feature_key_id(key):
    return "%s-%d%s%s" % (key[1], key[2], "-lens" if key[3] else "", "-" + key[4] if key[4] else "")


def feature_case(key):
    import mesh_scenes as ms
    import sphere_scenes as ss
    from raymond_amd.scene import CameraSettings, Settings, Transform

    kind, name, seed, lens, edge = key
    scene, cam, st, _ = (ss if kind == "spheres" else ms).build((name, seed, lens))
    use_dof = bool(st.use_dof)
    if edge is not None:
        focal, aperture = LENS_EDGES[edge]
        assert cam.transform.position == (0.0, 0.0, 0.0) and cam.fov_vert == 55.0
        cam, use_dof = CameraSettings(EDGE_FRAME[0], EDGE_FRAME[1], 55.0, Transform((0.0, 0.0, 0.0)), focal_length=focal, aperture_radius=aperture), True
    settings = Settings(cam, sample_count=FEATURE_SPP, bounce_limit=1, seed=st.seed, use_dof=use_dof)
    tunables = ms.scene_tunables((name, seed, lens)) if kind == "mesh" else {}
    return FeatureCase(key, scene, cam, settings, st.seed, use_dof, 5 if seed % 2 else 0, FEATURE_SPP, tunables)


@functools.lru_cache(maxsize=None)
def reference(key):
    """the composition's sums and term scales of a feature case: computed once per process, shared, read-only"""
    fc = feature_case(key)
    ref = Reference(*first_hit_sums(fc.scene, fc.cam, fc.seed, fc.spp, fc.begin, use_dof=fc.use_dof, scales=True))
    for a in ref:
        a.setflags(write=False)
    return ref


# ---------------------------------------------------------------- the one way out: a pixel off the bar because ONE sample's first hit is fragile
def candidates(scene, ray):
    """Every candidate hit of one ray, primitive by primitive through the oracle's own tests (every triangle of every grid object, not the walk)
    -> [(t, object, triangle)]"""
    L = O.load()
    objs, _, descs, _, _keep = scene.flatten()
    ray = np.ascontiguousarray(ray, dtype=np.float64).reshape(1, 6)
    out = []
    for i, o in enumerate(objs):
        if o.geometry_kind == 2:
            g = descs[o.grid_index]
            n = int(g.n_tris)
            tp = np.ascontiguousarray(np.ctypeslib.as_array(C.cast(g.tri_pos, C.POINTER(C.c_double)), (n, 9)))
            rays, hit, t = np.ascontiguousarray(np.tile(ray, (n, 1))), np.zeros(n, dtype=np.int32), np.zeros(n)
            L.orc_triangle_intersect(n, O.ptr(tp), O.ptr(rays), O.ptr(hit), O.ptr(t))
            out += [(float(t[k]), i, int(k)) for k in np.flatnonzero(hit)]
            continue
        hit, t = np.zeros(1, dtype=np.int32), np.zeros(1)
        if o.geometry_kind == 0:
            prim = np.array(list(o.origin) + list(o.normal))
            L.orc_plane_intersect(1, O.ptr(prim), O.ptr(ray), O.ptr(hit), O.ptr(t))
        else:
            prim = np.array(list(o.origin) + [o.radius])
            L.orc_sphere_intersect(1, O.ptr(prim), O.ptr(ray), O.ptr(hit), O.ptr(t))
        if hit[0]:
            out.append((float(t[0]), i, 0))
    return out


def fragile_hit(scene, osc, ray, obj, t, sub):
    """Why a device may legitimately see another first hit than the oracle's (obj, t, sub) on `ray` -> "tied", "grazing" or None.
    tied: a second candidate lies within 1e-9 relative of the hit in t.  grazing: the oracle's own answer (object and triangle, or the miss)
    changes when the ray's direction or origin is moved by 1e-9 of its size along an axis — the hit hangs on less than the bar."""
    if obj >= 0:
        for (t2, o2, s2) in candidates(scene, ray):
            if (o2, s2) != (int(obj), int(sub)) and abs(t2 - t) <= 1e-9 * max(abs(t), abs(t2)):
                return "tied"
    ray = np.asarray(ray, dtype=np.float64)
    moved = []
    for k in range(3):
        for sign in (-1.0, 1.0):
            d = ray[3:].copy()
            d[k] += sign * 1e-9
            moved.append(np.concatenate([ray[:3], d / np.sqrt((d * d).sum())]))
            o = ray[:3].copy()
            o[k] += sign * 1e-9 * max(1.0, float(np.abs(o).max()))
            moved.append(np.concatenate([o, ray[3:]]))
    obj2, _, sub2 = osc.scene_intersect(np.stack(moved))
    if ((obj2 != obj) | ((obj2 >= 0) & (sub2 != sub))).any():
        return "grazing"
    return None


def account_for_off_pixels(fc, dev, bad, run_sample, label, limit=3):
    """The one allowed way out of the per-pixel bar, after tests/test_gpu_fullsize.py's account_for_off_pixels (whose default limit on these frames
    is 3 pixels): every pixel of `dev` = (F, G) with a value in `bad` is traced again sample by sample — run_sample(x, y, s) -> the device's (F, G) of that one
    sample into a zeroed buffer over the 1 x 1 rect — and must be, bit for bit, the sequential sum of those samples; exactly ONE of its samples
    may differ from the oracle's, and that sample's oracle hit must be fragile (fragile_hit).  Anything else fails.  -> the number of pixels."""
    ys, xs = np.nonzero(bad.any(axis=2))
    assert len(ys) <= limit, "%s: %d pixels are outside the bar, first at (y, x) %s" % (label, len(ys), (int(ys[0]), int(xs[0])))
    osc = O.OracleScene(fc.scene)
    for y, x in zip(ys.tolist(), xs.tolist()):
        sums, off = [np.zeros(7), np.zeros(7)], []
        for s in range(fc.begin, fc.begin + fc.spp):
            d = run_sample(x, y, s)
            phi, obj, t, sub, ok, rays = sample_features(fc.scene, osc, fc.cam, fc.seed, fc.use_dof, [[x, y]], [s])
            one = (phi.reshape(1, 1, 7), (phi * phi).reshape(1, 1, 7))
            scale = (group_max(np.abs(one[0])), group_max(one[1]))
            if any(outside_the_pixel_bar(np.asarray(d[j]).reshape(1, 1, 7), one[j], scale[j]).any() for j in (0, 1)):
                off.append((s, int(obj[0]), float(t[0]), int(sub[0]), rays[0]))
            sums = [sums[j] + np.asarray(d[j]).reshape(7) for j in (0, 1)]
        for j in (0, 1):
            same = (sums[j].view(np.uint64) == np.ascontiguousarray(dev[j][y, x]).view(np.uint64)) | (np.isnan(sums[j]) & np.isnan(dev[j][y, x]))
            assert same.all(), "%s: pixel (%d, %d) is not the sum of its samples" % (label, x, y)
        assert len(off) == 1, "%s: pixel (%d, %d) is off the bar through %d samples: %s" % (label, x, y, len(off), [o[:4] for o in off])
        s, obj, t, sub, ray = off[0]
        why = fragile_hit(fc.scene, osc, ray, obj, t, sub)
        print("%s: pixel (%d, %d) sample %d off the bar: the oracle's hit (object %d, triangle %d, t %r) is %s" % (label, x, y, s, obj, sub, t, why))
        assert why is not None, "%s: pixel (%d, %d) sample %d differs from the oracle on a hit that is neither grazing nor tied" % (label, x, y, s)
    return len(ys)
