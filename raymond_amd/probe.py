"""Python wrappers of the diagnostic probes (include/raymond_hip_probe.h) for the parity tests."""
import ctypes as C
import os

import numpy as np

from . import abi
from . import lib as _lib

_vp = C.c_void_p
_sz = C.c_size_t
_P = C.POINTER
_SIGS = {
    "rmd_probe_philox4x32_10": [_vp, _sz, _vp, _vp, _vp],
    "rmd_probe_block_uniforms": [_vp, C.c_uint64, _sz, _vp, _vp, _vp, _vp],
    "rmd_probe_sphere_intersect": [_vp, _sz, _vp, _vp, _vp, _vp],
    "rmd_probe_sphere_normal": [_vp, _sz, _vp, _vp, _vp, _vp],
    "rmd_probe_plane_intersect": [_vp, _sz, _vp, _vp, _vp, _vp],
    "rmd_probe_aabb_intersect": [_vp, _sz, _vp, _vp, _vp, _vp],
    "rmd_probe_triangle_intersect": [_vp, _sz, _vp, _vp, _vp, _vp],
    "rmd_probe_triangle_normal": [_vp, _sz, _vp, _vp, _vp, _vp, _vp],
    "rmd_probe_onb": [_vp, _sz, _vp, _vp, _vp],
    "rmd_probe_cosine_hemisphere": [_vp, _sz, _vp, _vp, _vp, _vp],
    "rmd_probe_importance_sample_ggx": [_vp, _sz, _vp, _vp, _vp, _vp, _vp],
    "rmd_probe_ggx_distribution": [_vp, _sz, _vp, _vp, _vp, _vp],
    "rmd_probe_geometry_smith": [_vp, _sz, _vp, _vp, _vp, _vp, _vp],
    "rmd_probe_fresnel_schlick": [_vp, _sz, _vp, _vp, _vp],
    "rmd_probe_primary_ray": [_vp, _sz, _P(abi.Camera), _vp, _vp, _vp],
    "rmd_probe_elementary": [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "rmd_probe_scene_intersect": [_vp, _vp, _sz, _vp, _vp, _vp, _vp],
    "rmd_probe_grid_intersect": [_vp, _vp, C.c_uint32, _sz, _vp, _vp, _vp, _vp],
    "rmd_probe_grid_intersect_deep": [_vp, _vp, C.c_uint32, _sz, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp],
    "rmd_probe_trace_samples": [_vp, _vp, _P(abi.Camera), _P(abi.Settings), _sz, _vp, _vp, _vp, _vp, _vp],
    "rmd_probe_triangle_sphere": [_sz, _vp, _vp],
    "rmd_probe_pretest_pairs": [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "rmd_probe_primary_candidates": [_P(abi.Camera), _P(abi.Settings), _P(abi.Object), C.c_uint32, C.c_uint32, C.c_int64, _sz, _vp, _vp, _vp],
    "rmd_probe_tile_classes": [_P(abi.Camera), _P(abi.Settings), _P(abi.Object), C.c_uint32, C.c_uint32, C.c_int64, _sz, _vp, _vp, _vp],
    "rmd_probe_launch_plan": [C.c_uint32, C.c_uint32, _sz, _vp, _vp],
    "rmd_probe_launch_sizes": [C.c_uint32, C.c_uint32, _vp],
    "rmd_probe_work_plan": [_vp, _sz, _vp, _vp],
    "rmd_probe_work_items": [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _sz, _vp, _P(C.c_uint32)],
    "rmd_probe_scene_layout": [_vp, _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32)],
    "rmd_probe_scene_plan": [_vp, _vp, _sz, _vp],
    "rmd_probe_rays_plan": [_vp, C.c_uint64, _vp],
    "rmd_probe_denoise_scratch": [C.c_uint32] * 6 + [C.c_uint64, _vp, _P(C.c_uint64)],
    "rmd_probe_feature_slope": [_vp, _vp, C.c_uint32, C.c_uint32, C.c_double, _vp],
    "rmd_probe_atrous_region_slope_planes": [_vp, C.c_uint32, C.c_uint32, _vp],
    "rmd_probe_denoise_scratch_slope": [C.c_uint32] * 7 + [C.c_uint64, _vp, _P(C.c_uint64)],
    "rmd_probe_denoise_tile": [C.c_uint32, C.c_uint32, _vp],
}
PATH_STRIDE = 17
_ready = False


PROBE_LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libraymond_hip_probe.so")  # beside the product library it links against
_probe_lib = None


def _L():
    """libraymond_hip_probe.so: test infrastructure, a library of its own (the product library exports no probe)."""
    global _ready, _probe_lib
    if not _ready:
        _lib.load()  # the product library first: the probes call into it
        if not os.path.exists(PROBE_LIB_PATH):
            raise ImportError("raymond_amd.probe: %s is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'`" % PROBE_LIB_PATH)
        _probe_lib = C.CDLL(PROBE_LIB_PATH)
        for name, args in _SIGS.items():
            fn = getattr(_probe_lib, name)
            fn.restype, fn.argtypes = C.c_int32, args
        _ready = True
    return _probe_lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f(a, w=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if w is None else a.reshape(-1, w)


def hit_t(ctx, name, shape, rays):
    """sphere/plane/aabb/triangle intersect -> (hit int32[n], t float64[n])"""
    L = _L()
    rays = _f(rays, 6)
    shape = _f(shape).reshape(rays.shape[0], -1)
    n = rays.shape[0]
    hit = np.zeros(n, dtype=np.int32)
    t = np.zeros(n)
    ctx.check(getattr(L, "rmd_probe_%s_intersect" % name)(ctx.handle, n, _p(shape), _p(rays), _p(hit), _p(t)))
    return hit, t


def call(ctx, name, n, ins, outs):
    """generic: ins = list of float64 arrays, outs = list of output widths"""
    L = _L()
    ins = [_f(a) for a in ins]
    res = [np.zeros((n, w)) for w in outs]
    ctx.check(getattr(L, "rmd_probe_" + name)(ctx.handle, n, *[_p(a) for a in ins], *[_p(a) for a in res]))
    return res


def philox(ctx, ctr, key):
    L = _L()
    ctr = np.ascontiguousarray(ctr, dtype=np.uint32).reshape(-1, 4)
    key = np.ascontiguousarray(key, dtype=np.uint32).reshape(-1, 2)
    out = np.zeros_like(ctr)
    ctx.check(L.rmd_probe_philox4x32_10(ctx.handle, ctr.shape[0], _p(ctr), _p(key), _p(out)))
    return out


def block_uniforms(ctx, seed, pixel, sample, block):
    """-> (n, 5): u53_0, u53_1 of the block as next2() returns them, then r (22-bit), r1, r2 as next3() returns them"""
    L = _L()
    pixel, sample, block = (np.ascontiguousarray(a, dtype=np.uint32) for a in (pixel, sample, block))
    out = np.zeros((pixel.shape[0], 5))
    ctx.check(L.rmd_probe_block_uniforms(ctx.handle, seed, pixel.shape[0], _p(pixel), _p(sample), _p(block), _p(out)))
    return out


def elementary(ctx, x):
    """-> (sqrt64(x), sin(x), cos(x), root, 1/root) as the device computes them (root, 1/root: normalize()'s pair)"""
    L = _L()
    x = _f(x).ravel()
    s, si, co, ro, ir = (np.zeros_like(x) for _ in range(5))
    ctx.check(L.rmd_probe_elementary(ctx.handle, x.shape[0], _p(x), _p(s), _p(si), _p(co), _p(ro), _p(ir)))
    return s, si, co, ro, ir


def primary_ray(ctx, cam, xy, u):
    L = _L()
    xy = np.ascontiguousarray(xy, dtype=np.uint32).reshape(-1, 2)
    u = _f(u, 2)
    out = np.zeros((xy.shape[0], 6))
    c = cam.pod()
    ctx.check(L.rmd_probe_primary_ray(ctx.handle, xy.shape[0], C.byref(c), _p(xy), _p(u), _p(out)))
    return out


def scene_intersect(ctx, dscene, rays):
    L = _L()
    rays = _f(rays, 6)
    n = rays.shape[0]
    obj = np.zeros(n, dtype=np.int32)
    t = np.zeros(n)
    sub = np.zeros(n, dtype=np.uint32)
    ctx.check(L.rmd_probe_scene_intersect(ctx.handle, dscene.handle, n, _p(rays), _p(obj), _p(t), _p(sub)))
    return obj, t, sub


def grid_intersect(ctx, dscene, g, rays):
    L = _L()
    rays = _f(rays, 6)
    n = rays.shape[0]
    hit = np.zeros(n, dtype=np.int32)
    t = np.zeros(n)
    tri = np.zeros(n, dtype=np.uint32)
    ctx.check(L.rmd_probe_grid_intersect(ctx.handle, dscene.handle, g, n, _p(rays), _p(hit), _p(t), _p(tri)))
    return hit, t, tri


def grid_intersect_deep(ctx, dscene, g, rays, cut_lanes=0, cut_round=0, rays_per_wave=64):
    """AccGrid::intersects through the DEEP form of the walk (pre-test, ring, walks put aside and taken up again), one wave per `rays_per_wave`
    consecutive rays.  api: rmd_probe_grid_intersect_deep."""
    L = _L()
    rays = _f(rays, 6)
    n = rays.shape[0]
    hit = np.zeros(n, dtype=np.int32)
    t = np.zeros(n)
    tri = np.zeros(n, dtype=np.uint32)
    ctx.check(L.rmd_probe_grid_intersect_deep(ctx.handle, dscene.handle, g, n, _p(rays), cut_lanes, cut_round, rays_per_wave, _p(hit), _p(t), _p(tri)))
    return hit, t, tri


def trace_samples(ctx, dscene, cam, settings, xy, samples, paths=False):
    L = _L()
    xy = np.ascontiguousarray(xy, dtype=np.uint32).reshape(-1, 2)
    samples = np.ascontiguousarray(samples, dtype=np.uint32)
    n = xy.shape[0]
    rgb = np.zeros((n, 3))
    po = np.full((n, PATH_STRIDE), -2, dtype=np.int32) if paths else None
    ps = np.zeros((n, PATH_STRIDE), dtype=np.uint32) if paths else None
    c, s = cam.pod(), settings.pod()
    ctx.check(
        L.rmd_probe_trace_samples(ctx.handle, dscene.handle, C.byref(c), C.byref(s), n, _p(xy), _p(samples), _p(rgb),
                                  _p(po) if paths else None, _p(ps) if paths else None)
    )
    return (rgb, po, ps) if paths else rgb


def triangle_sphere(pos9):
    """Host only (no GPU): the pre-test sphere of each triangle -> (centre float64[n, 3], r2a float64[n], kb float64[n]); api: rmd_probe_triangle_sphere."""
    from . import abi as _abi

    L = _L()
    pos9 = _f(pos9, 9)
    out = np.zeros((pos9.shape[0], 5))
    st = L.rmd_probe_triangle_sphere(pos9.shape[0], _p(pos9), _p(out))
    if st != _abi.RMD_OK:
        raise RuntimeError("rmd_probe_triangle_sphere: status %d" % st)
    return out[:, :3], out[:, 3], out[:, 4]


def pretest_pairs(ctx, sphere5, pos9, ray6):
    """The walk's sphere pre-test in the device's own arithmetic and the device's triangle test on explicit pairs -> (passed bool[n], hit bool[n],
    t float64[n]); sphere5 = centre, r2a, kb per pair.  api: rmd_probe_pretest_pairs."""
    L = _L()
    sphere5, pos9, ray6 = _f(sphere5, 5), _f(pos9, 9), _f(ray6, 6)
    n = pos9.shape[0]
    passed, hit, t = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n)
    ctx.check(L.rmd_probe_pretest_pairs(ctx.handle, n, _p(sphere5), _p(pos9), _p(ray6), _p(passed), _p(hit), _p(t)))
    return passed.astype(bool), hit.astype(bool), t


def primary_candidates(cam, settings, scene, tiles, axis_pairs_tunable=0):
    """Host only (no GPU): what the spheres kernel's generation trips visit for the primary rays of each wave tile (x0, y0, w, h) ->
    (launch_visit_mask int, launch_axis_pairs int, on bool, visit uint64[n], pairs uint32[n]); api: rmd_probe_primary_candidates."""
    L = _L()
    objs, n, _descs, ng, keep = scene.flatten()
    tiles = np.ascontiguousarray(tiles, dtype=np.uint32).reshape(-1, 4)
    launch, out = np.zeros(3, dtype=np.uint64), np.zeros((tiles.shape[0], 2), dtype=np.uint64)
    c, s = cam.pod(), settings.pod()
    st = L.rmd_probe_primary_candidates(C.byref(c), C.byref(s), objs, n, ng, int(axis_pairs_tunable), tiles.shape[0], _p(tiles), _p(launch), _p(out))
    del keep
    if st != abi.RMD_OK:
        raise RuntimeError("rmd_probe_primary_candidates: status %d" % st)
    return int(launch[0]), int(launch[1]), bool(launch[2]), out[:, 0].copy(), out[:, 1].astype(np.uint32)


TILE_GENERAL, TILE_EMITTER, TILE_BLACK = 0, 1, 2


def tile_classes(cam, settings, scene, tiles, axis_pairs_tunable=0):
    """Host only (no GPU): the class the spheres kernel gives a work item of each wave tile (x0, y0, w, h) ->
    (on bool, cls int32[n] (TILE_*), wall int32[n]: the object every primary ray of the tile hits, -1 = general); api: rmd_probe_tile_classes."""
    L = _L()
    objs, n, _descs, ng, keep = scene.flatten()
    tiles = np.ascontiguousarray(tiles, dtype=np.uint32).reshape(-1, 4)
    launch, out = np.zeros(1, dtype=np.uint32), np.zeros((tiles.shape[0], 2), dtype=np.int32)
    c, s = cam.pod(), settings.pod()
    st = L.rmd_probe_tile_classes(C.byref(c), C.byref(s), objs, n, ng, int(axis_pairs_tunable), tiles.shape[0], _p(tiles), _p(launch), _p(out))
    del keep
    if st != abi.RMD_OK:
        raise RuntimeError("rmd_probe_tile_classes: status %d" % st)
    return bool(launch[0]), out[:, 0].copy(), out[:, 1].copy()


# rmd_probe_launch_plan: modes, input flags and output columns
MODE_TILES, MODE_TILES_BUFFERED, MODE_LIST = 0, 1, 2
PLAN_QUEUES, PLAN_PERSIST, PLAN_CHAIN, PLAN_MOMENTS = 1, 2, 4, 8
PLAN_FIELDS = ("persistent", "queued", "chained", "moments", "waves_per_wg", "workgroups", "wave_lds", "lds")
SIZE_FIELDS = ("budget", "object", "wave", "queued_wave", "persist_waves", "grid_waves", "sort_pool", "mask_budget")


def _host_check(st, name):
    if st != abi.RMD_OK:
        raise RuntimeError("%s: status %d" % (name, st))


def launch_plan(mode, grid, n_objects, mask_words_total, flags, n_waves, n_cus):
    """Host only (no GPU): the form launch_render gives each launch -> dict of uint64 arrays keyed by PLAN_FIELDS; the inputs broadcast against
    each other.  api: rmd_probe_launch_plan."""
    L = _L()
    cols = np.broadcast_arrays(*(np.asarray(a, dtype=np.int64) for a in (n_objects, mask_words_total, flags, n_waves, n_cus)))
    inp = np.ascontiguousarray(np.stack([c.ravel() for c in cols], axis=1).astype(np.uint32))
    out = np.zeros((inp.shape[0], 8), dtype=np.uint64)
    _host_check(L.rmd_probe_launch_plan(mode, int(grid), inp.shape[0], _p(inp), _p(out)), "rmd_probe_launch_plan")
    return {k: out[:, i].astype(np.int64).reshape(cols[0].shape) for i, k in enumerate(PLAN_FIELDS)}


def launch_sizes(mode, grid):
    """Host only: the sizes of the launch plan of instantiation (mode, grid) -> dict keyed by SIZE_FIELDS.  api: rmd_probe_launch_sizes."""
    L = _L()
    out = np.zeros(8, dtype=np.uint64)
    _host_check(L.rmd_probe_launch_sizes(mode, int(grid), _p(out)), "rmd_probe_launch_sizes")
    return {k: int(v) for k, v in zip(SIZE_FIELDS, out)}


def work_plan(wave_slots, n_tiles, sample_count, k_uniform, ctx=None, pass_samples=0):
    """Host only: the two-part work list of the spheres kernel's split launches -> (n_whole, n_tail, k_tail) int64 arrays; the inputs broadcast
    against each other.  With a render.Context the plan is the one that context gives a pass of pass_samples samples (0: the only pass) of a render
    of n_tiles wave tiles and sample_count samples of a scene without grids (wave_slots and k_uniform are ignored).  api: rmd_probe_work_plan."""
    L = _L()
    if ctx is not None:
        wave_slots = pass_samples
    cols = np.broadcast_arrays(*(np.asarray(a, dtype=np.int64) for a in (wave_slots, n_tiles, sample_count, k_uniform)))
    inp = np.ascontiguousarray(np.stack([c.ravel() for c in cols], axis=1).astype(np.uint32))
    out = np.zeros((inp.shape[0], 3), dtype=np.uint32)
    _host_check(L.rmd_probe_work_plan(ctx.handle if ctx is not None else None, inp.shape[0], _p(inp), _p(out)), "rmd_probe_work_plan")
    return tuple(out[:, i].astype(np.int64).reshape(cols[0].shape) for i in range(3))


WORK_ITEM_FIELDS = ("tile", "first", "count", "parts", "whole")


def work_items(n_tiles, n_whole, k_tail, sample_count, extra=0):
    """Host only: every item of the list, and `extra` numbers past its end, by the mapping the kernel evaluates -> (int64 array [items + extra, 5]
    in the order of WORK_ITEM_FIELDS, the number of items).  api: rmd_probe_work_items."""
    L = _L()
    n_items = C.c_uint32()
    _host_check(L.rmd_probe_work_items(n_tiles, n_whole, k_tail, sample_count, 0, 0, None, C.byref(n_items)), "rmd_probe_work_items")
    out = np.zeros((n_items.value + extra, 5), dtype=np.uint32)
    _host_check(L.rmd_probe_work_items(n_tiles, n_whole, k_tail, sample_count, 0, out.shape[0], _p(out), C.byref(n_items)), "rmd_probe_work_items")
    return out.astype(np.int64), n_items.value


def scene_layout(dscene):
    """(n_objects, n_grids, mask_words_total) of an uploaded scene.  api: rmd_probe_scene_layout."""
    L = _L()
    n, g, m = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _host_check(L.rmd_probe_scene_layout(dscene.handle, C.byref(n), C.byref(g), C.byref(m)), "rmd_probe_scene_layout")
    return n.value, g.value, m.value


RAYS_PLAN_FIELDS = ("batches", "waves_per_wg", "workgroups", "total_waves", "lds", "n_cus")


def rays_plan(dscene, n_rays):
    """The launch rmd_intersect_rays would make for `n_rays` rays on an uploaded scene -> dict keyed by RAYS_PLAN_FIELDS.  api: rmd_probe_rays_plan."""
    L = _L()
    out = np.zeros(6, dtype=np.uint64)
    _host_check(L.rmd_probe_rays_plan(dscene.handle, int(n_rays), _p(out)), "rmd_probe_rays_plan")
    return dict(zip(RAYS_PLAN_FIELDS, (int(v) for v in out)))


SCENE_PLAN_FIELDS = ("n_grid_objects", "regular", "walk_steps_bound", "axis_pairs", "visit_mask", "grid_mask", "n_grids")


def scene_plan(dscene):
    """What rmd_scene_create decided once for an uploaded scene -> dict keyed by SCENE_PLAN_FIELDS, plus "mask_shift" and "mask_bits": one int per
    grid.  api: rmd_probe_scene_plan."""
    L = _L()
    out = np.zeros(8, dtype=np.uint64)
    _host_check(L.rmd_probe_scene_plan(dscene.handle, _p(out), 0, None), "rmd_probe_scene_plan")
    n = int(out[6])
    per_grid = np.zeros((max(n, 1), 2), dtype=np.uint32)
    _host_check(L.rmd_probe_scene_plan(dscene.handle, _p(out), n, _p(per_grid)), "rmd_probe_scene_plan")
    plan = {k: int(v) for k, v in zip(SCENE_PLAN_FIELDS, out)}
    plan["mask_shift"], plan["mask_bits"] = [int(v) for v in per_grid[:n, 0]], [int(v) for v in per_grid[:n, 1]]
    return plan


def feature_slope(ctx, f, fvalid, slope):
    """The device's slope floors of (H, W, 7) feature means `f` with the (H, W) feature-validity mask -> m (H, W, 7).  api: rmd_probe_feature_slope."""
    L = _L()
    H, W = fvalid.shape
    planes = np.ascontiguousarray(np.moveaxis(np.asarray(f, dtype=np.float64), -1, 0)).copy()
    planes[0][~np.asarray(fvalid, dtype=bool)] = np.nan  # the mark feature_planes_pixel leaves
    out = np.zeros_like(planes)
    ctx.check(L.rmd_probe_feature_slope(ctx.handle, _p(planes), W, H, float(slope), _p(out)))
    return np.moveaxis(out, 0, -1).copy()


def atrous_region_slope_planes(ctx, width, height):
    """The slope planes the context's last sloped rmd_denoise_atrous_dual_slope_region call left in its scratch -> m (H, W, 7); defined on level 0's needed
    set only.  api: rmd_probe_atrous_region_slope_planes."""
    out = np.zeros((7, height, width), dtype=np.float64)
    ctx.check(_L().rmd_probe_atrous_region_slope_planes(ctx.handle, width, height, _p(out)))
    return np.moveaxis(out, 0, -1).copy()


# rmd_probe_denoise_scratch: the forms, and the parts in the order of denoise_host.hpp's ScratchPart
SCRATCH_FORMS = ("single", "atrous", "dual", "atrous_dual", "atrous_dual_region", "dual_select", "tile_error")
SCRATCH_PARTS = ("planes", "f_b", "cand_img", "gain", "feat_planes", "n_img", "win_img", "n_f_img", "table", "rects", "counts_a", "counts_b", "counts_f",
                 "tile_errors", "slope_planes")


def denoise_scratch(form, width, height, n_rects, guided=False, n_cands=0, n_table=0, sloped=None, atrous_sloped=None):
    """Host only: the scratch block of a denoise call -> ({part: (offset, bytes)} of the parts the form holds, total bytes).  sloped (None: the call
    has no slope argument): a non-local-means _slope call, and whether a slope it reads is > 0.  atrous_sloped (None likewise): an a-trous _slope call
    (rmd_denoise_atrous_slope, rmd_denoise_atrous_dual_slope[_region]), and whether its slope is > 0.
    api: rmd_probe_denoise_scratch, rmd_probe_denoise_scratch_slope."""
    if atrous_sloped is not None:
        assert sloped is None, "one call has one slope"
        sloped = 2 if atrous_sloped else 0
    L = _L()
    out = np.zeros((len(SCRATCH_PARTS), 3), dtype=np.uint64)
    total = C.c_uint64()
    if sloped is None:
        _host_check(L.rmd_probe_denoise_scratch(SCRATCH_FORMS.index(form), width, height, n_rects, int(guided), n_cands, n_table, _p(out), C.byref(total)),
                    "rmd_probe_denoise_scratch")
    else:
        _host_check(L.rmd_probe_denoise_scratch_slope(SCRATCH_FORMS.index(form), width, height, n_rects, int(guided), int(sloped), n_cands, n_table, _p(out),
                                                      C.byref(total)), "rmd_probe_denoise_scratch_slope")
    return {name: (int(o), int(b)) for name, (used, o, b) in zip(SCRATCH_PARTS, out) if used}, total.value


def denoise_tile(radius, patch_radius):
    """Host only: the non-local-means kernels' workgroup tile at a window -> (tile width, its LDS bytes, the 32-wide tile's LDS bytes, the LDS budget), from
    the functions the launchers size their launch with.  api: rmd_probe_denoise_tile."""
    out = np.zeros(4, dtype=np.uint64)
    _host_check(_L().rmd_probe_denoise_tile(int(radius), int(patch_radius), _p(out)), "rmd_probe_denoise_tile")
    return tuple(int(v) for v in out)
