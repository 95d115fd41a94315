"""Launch forms at the edges of the LDS budget, on the GPU.  tests/test_launch_plan.py checks the plan (render_kernel.hpp: plan_launch) on the host;
this renders scenes placed either side of each of its boundaries — a small mesh or the spheres-only scene plus k extra spheres — and checks that
the launch made is the plan's, that every form gives the same frame bit for bit, and, at one point per former failure window, the oracle's.
The second test takes the queued form's fallback: a device that cannot provide the path queues renders with the lane-per-path kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

from raymond_amd import abi, lib, probe, render, scenes
from raymond_amd.scene import Material, Object, Settings, Sphere, generate_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "raymond_amd", "csrc", "diag", "libraymond_hip.so")
TILES, BUFFERED = probe.MODE_TILES, probe.MODE_TILES_BUFFERED
W, H, SPP, SPLIT = 44, 30, 8, 2  # a ragged frame: partial wave tiles on both axes


def rel_close(a, b, rtol):
    scale = np.maximum(np.abs(a), np.abs(b))
    return (np.abs(a - b) <= rtol * np.maximum(scale, 1e-300)) | (np.isnan(a) & np.isnan(b)) | (a == b)


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def base_scene(kind):
    return scenes.mesh_scene(scenes.lumpy_sphere_mesh(13)) if kind == "mesh" else scenes.reflective_spheres()


def with_spheres(kind, k):
    sc = base_scene(kind)
    rng = np.random.default_rng(k)
    for i in range(k):
        c = (rng.uniform(-1.8, 1.8), rng.uniform(-0.9, 1.8), rng.uniform(1.5, 4.8))
        mat = Material.Metal(tuple(rng.uniform(0.2, 1.0, 3)), 0.05) if i % 3 == 0 else Material.Diffuse(tuple(rng.uniform(0.0, 1.0, 3)), 0.3)
        sc.objects.append(Object(Sphere(c, rng.uniform(0.02, 0.06)), mat))
    return sc


def sweep_points(kind, n0, m):
    """k at -1 / +1 of every boundary of the forced persistent split launch, from the sizes: X(k) = 128 (n0 + k) + 4 round4(m) is the LDS of the
    table and the masks, and a boundary b is crossed between the last k with X <= b and the next.  Returns {k: label}."""
    grid = kind == "mesh"
    S = probe.launch_sizes(BUFFERED, grid)
    B, obj, fixed0 = S["budget"], S["object"], 4 * ((m + 3) // 4 * 4)
    pwave = S["queued_wave"] if grid else S["wave"]  # the persistent split launch of a mesh scene runs with path queues
    edges = {"persistent %d -> %d waves" % (w, w - 1): B - w * pwave for w in range(S["persist_waves"], 4, -1)}
    edges["one wave per item"] = B - 4 * pwave
    if grid:
        for w in (4, 3, 2):
            edges["one wave per item, %d -> %d waves" % (w, w - 1)] = B - w * S["wave"]
        for w in (3, 2, 1):
            edges["window of %d waves" % w] = B - w * pwave  # (the queued pricing's edge: where a fallback charged at it stopped fitting)
    edges["admission"] = B - S["wave"]  # one unqueued wave beside the table (the spheres kernel's: its pool and its head)
    points = {}
    for label, b in edges.items():
        k_lo = (b - fixed0) // obj - n0
        for k, side in ((k_lo, "-"), (k_lo + 1, "+")):
            if k >= 0:
                points.setdefault(int(k), []).append(side + label)
    return dict(sorted(points.items()))


def plan_of(mode, grid, n, m, flags):
    p = probe.launch_plan(mode, grid, [n], [m], flags, 1, 1)
    return {k: int(v[0]) for k, v in p.items()}


def check_info(info, plan, where):
    got = (info.persistent, info.queued, info.chained, info.waves_per_workgroup)
    want = (plan["persistent"], plan["queued"], plan["chained"], plan["waves_per_wg"])
    assert got == want, (where, got, want)


def render_form(ctx, ds, st, tiles, fb, tunables, fb_sq=None):
    for key, v in tunables.items():
        ctx.set_tunable(key, v)
    try:
        fb.zero()
        if fb_sq is not None:
            fb_sq.zero()
        render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fb, framebuffer_sq=fb_sq)
        return fb.download(), ctx.last_launch_info()
    finally:
        for key in tunables:
            ctx.set_tunable(key, 0)


def ordered_sums(ctx, ds, st):
    """numpy's sum and sum of squares of every pixel's samples 0 .. SPP-1, added in sample order, from the list-mode probe."""
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1), SPP, axis=0)
    smp = np.tile(np.arange(SPP, dtype=np.uint32), W * H)
    L = probe.trace_samples(ctx, ds, st.camera_settings, st, xy, smp).reshape(H * W, SPP, 3)
    S, Q = np.zeros((H * W, 3)), np.zeros((H * W, 3))
    for s in range(SPP):
        S = S + L[:, s]
        Q = Q + L[:, s] * L[:, s]
    return S.reshape(H, W, 3), Q.reshape(H, W, 3)


@pytest.mark.parametrize("kind", ["mesh", "spheres"])
def test_launch_forms_either_side_of_every_lds_boundary(gpu_ctx, oracle, kind):
    """At each point: the forced persistent split launch (with path queues for the mesh) is the plan's launch, and equals the direct mode and — mesh
    scenes — the lane-per-path split launch (RMD_TUNE_PATH_QUEUES = 1) bit for bit.  The last admitted scene renders, the next is refused with
    RMD_ERR_UNSUPPORTED before anything is launched.  Spheres-kernel points, and one mesh point in direct mode, also render with the squares: the sum
    is the plain frame's bits and the squares numpy's ordered sum of the probe's samples."""
    grid = kind == "mesh"
    st = Settings(scenes.camera(W, H), sample_count=SPP, bounce_limit=4, seed=7)
    tiles = generate_tiles(W, H, (32, 32))
    fb, fb_sq = render.Framebuffer(gpu_ctx, W, H), render.Framebuffer(gpu_ctx, W, H)
    ds0 = render.DeviceScene(gpu_ctx, base_scene(kind))
    n0, g0, m = probe.scene_layout(ds0)
    ds0.close()
    assert (g0 != 0) == grid and (m != 0) == (g0 != 0) and m % 4 == 0, (n0, g0, m)  # grids exactly when mask words: what the plan sizes by
    points = sweep_points(kind, n0, m)
    admission = [k for k, labels in points.items() if "+admission" in labels]
    oracle_for = {}  # one point inside each former failure window (its lower edge + 1)
    mesh_moments_done = False
    log = []
    split_flags = probe.PLAN_PERSIST | (probe.PLAN_QUEUES | probe.PLAN_CHAIN if grid else 0)
    for k, labels in points.items():
        sc = with_spheres(kind, k)
        ds = render.DeviceScene(gpu_ctx, sc)
        try:
            n, g, mk = probe.scene_layout(ds)
            assert (n, g, mk) == (n0 + k, g0, m), (k, n, g, mk)
            if k in admission:
                gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, SPLIT), gpu_ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 2)
                try:
                    with pytest.raises(lib.RaymondError) as e:
                        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb)
                finally:
                    gpu_ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0), gpu_ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 0)
                assert e.value.status == abi.RMD_ERR_UNSUPPORTED, (k, str(e.value))
                log.append("k=%d %s: refused" % (k, ",".join(labels)))
                continue
            where = "%s k=%d %s" % (kind, k, ",".join(labels))
            split_frame, info = render_form(gpu_ctx, ds, st, tiles, fb, {abi.RMD_TUNE_SAMPLE_SPLIT: SPLIT, abi.RMD_TUNE_LAUNCH_FORM: 2})
            assert info.buffered == 1 and info.split_k == SPLIT and info.has_grid == grid, where
            plan = plan_of(BUFFERED, grid, n, mk, split_flags)
            check_info(info, plan, where)
            log.append("k=%d %s: persistent %d queued %d chained %d waves %d" % (k, ",".join(labels), info.persistent, info.queued, info.chained, info.waves_per_workgroup))
            direct, dinfo = render_form(gpu_ctx, ds, st, tiles, fb, {abi.RMD_TUNE_SAMPLE_SPLIT: 1, abi.RMD_TUNE_LAUNCH_FORM: 2})
            assert dinfo.buffered == 0, where
            check_info(dinfo, plan_of(TILES, grid, n, mk, probe.PLAN_PERSIST), where + " direct")
            assert same_bits(split_frame, direct), where + ": the split launch differs from the direct mode"
            if grid:
                lane, linfo = render_form(gpu_ctx, ds, st, tiles, fb, {abi.RMD_TUNE_SAMPLE_SPLIT: SPLIT, abi.RMD_TUNE_LAUNCH_FORM: 2, abi.RMD_TUNE_PATH_QUEUES: 1})
                check_info(linfo, plan_of(BUFFERED, grid, n, mk, probe.PLAN_PERSIST | probe.PLAN_CHAIN), where + " no queues")
                assert same_bits(split_frame, lane), where + ": the lane-per-path split launch differs"
                for label in labels:
                    if label.startswith("+window") or label == "+one wave per item":
                        oracle_for.setdefault(label, (k, sc, split_frame))
            if not grid or not mesh_moments_done:
                tun = {abi.RMD_TUNE_SAMPLE_SPLIT: SPLIT, abi.RMD_TUNE_LAUNCH_FORM: 2} if not grid else {abi.RMD_TUNE_SAMPLE_SPLIT: 1, abi.RMD_TUNE_LAUNCH_FORM: 2}
                acc, minfo = render_form(gpu_ctx, ds, st, tiles, fb, tun, fb_sq)
                mode = BUFFERED if not grid else TILES
                check_info(minfo, plan_of(mode, grid, n, mk, probe.PLAN_PERSIST | probe.PLAN_MOMENTS), where + " moments")
                assert same_bits(acc, split_frame), where + ": the moments launch changed the sum"
                S, Q = ordered_sums(gpu_ctx, ds, st)
                assert same_bits(acc, S) and same_bits(fb_sq.download(), Q), where + ": the squares differ from the ordered sum of the samples"
                mesh_moments_done = True
        finally:
            ds.close()
    fb.close(), fb_sq.close()
    print("\n".join(log))
    assert len(admission) == 1
    if grid:
        assert sorted(oracle_for) == ["+one wave per item", "+window of 1 waves", "+window of 2 waves", "+window of 3 waves"], sorted(oracle_for)
    for label, (k, sc, frame) in oracle_for.items():
        ref = oracle.OracleScene(sc).render_tiles(st.camera_settings, st, tiles, threads=8)
        ok = rel_close(frame, ref, 1e-9).all(axis=2)
        assert ok.mean() >= 0.995, (label, k, (~ok).sum())


QUEUE_CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np
from raymond_amd import abi, lib, render, scenes
from raymond_amd.scene import Settings, generate_tiles

assert lib.LIB_PATH.endswith("diag/libraymond_hip.so"), lib.LIB_PATH
W, H = 64, 48
sc = scenes.mesh_scene(scenes.lumpy_sphere_mesh(13))
st = Settings(scenes.camera(W, H), sample_count=8, bounce_limit=4, seed=3)
tiles = generate_tiles(W, H, (32, 32))

def frame(ctx):
    ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 2), ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 2)
    ds, fb = render.DeviceScene(ctx, sc), render.Framebuffer(ctx, W, H)
    render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fb)
    img, info = fb.download(), ctx.last_launch_info()
    fb.close(), ds.close()
    return img, info

os.environ.pop("RMD_DEBUG", None)
with render.Context(0) as ctx:
    queued, info = frame(ctx)
    assert (info.persistent, info.queued, info.buffered) == (1, 1, 1), (info.persistent, info.queued)
os.environ["RMD_DEBUG"] = "256"  # read once, when the context is created: the path queues' allocation reports hipErrorOutOfMemory
with render.Context(0) as ctx:
    for attempt in range(2):  # the fallback, then a second launch on the same context: clean, and the same frame again
        img, info = frame(ctx)
        assert (info.persistent, info.queued, info.buffered, info.chained) == (1, 0, 1, 1), (attempt, info.persistent, info.queued, info.chained)
        assert img.tobytes() == queued.tobytes(), "the lane-per-path fallback differs from the queued frame"
        ctx.synchronize()
print("queue fallback ok")
"""


def test_the_path_queue_fallback_renders_the_queued_frame(product_lib):
    """api.cpp: a device that cannot allocate the path queues (~239 MB) runs the persistent split launch with the lane-per-path kernel.  The DIAG
    build's RMD_DEBUG bit 256 makes that allocation report hipErrorOutOfMemory — no memory is taken from the shared device to get there."""
    assert os.path.exists(DIAG_LIB), "build the DIAG library: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, RAYMOND_HIP_LIB=DIAG_LIB)
    env.pop("RMD_DEBUG", None)
    r = subprocess.run([sys.executable, "-c", QUEUE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "queue fallback ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
