"""The expected sums of rmd_render_features, composed from the oracle's existing entry points and nothing else:
orc_block_uniforms (block 0) -> orc_primary_ray -> orc_scene_intersect -> the plane's stored normal / orc_sphere_normal / orc_triangle_normal,
the material's colour and t; sequential sums in sample order.  Pinhole rays only (the oracle has no thin-lens entry point)."""
import ctypes as C

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


def first_hit_sums(scene, cam, seed, spp, sample_begin=0):
    """-> F, G (H, W, 7): the sums and sums of squares of the first-hit features of samples sample_begin .. + spp - 1, and the per-sample object
    indices (spp, H, W)."""
    L = O.load()
    W, H = cam.backbuffer_width, cam.backbuffer_height
    c = cam.pod()
    osc = O.OracleScene(scene)
    xy, pix = pixel_grid(W, H)
    F, G = np.zeros((H, W, 7)), np.zeros((H, W, 7))
    objs = []
    for s in range(sample_begin, sample_begin + spp):
        u = np.ascontiguousarray(O.block_uniforms(seed, pix, [s] * len(pix), [0] * len(pix))[:, :2])
        rays = np.zeros((len(pix), 6))
        L.orc_primary_ray(len(pix), C.byref(c), O.ptr(xy), O.ptr(u), O.ptr(rays))
        obj, t, sub = osc.scene_intersect(rays)
        f = hit_features(scene, rays, obj, t, sub).reshape(H, W, 7)
        F = F + f
        G = G + f * f
        objs.append(obj.reshape(H, W).copy())
    return F, G, np.stack(objs)


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
