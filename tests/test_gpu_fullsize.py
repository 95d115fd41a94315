"""GPU checks at BASELINE.json's full configuration sizes (1920x1080, the 99,372-triangle stand-in, 5 and 8 bounces,
thin lens), through size-independent properties and oracle spot checks — the oracle cannot render these sizes in
test time, the GPU can."""
import ctypes as C

import numpy as np
import pytest

from raymond_amd import abi, probe, render, scenes
from raymond_amd.scene import Settings, generate_tiles

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dragon(product_lib):
    return scenes.gold_dragon_standin()


def rel_close(a, b, rtol):
    return (np.abs(a - b) <= rtol * np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)) | (a == b) | (np.isnan(a) & np.isnan(b))


def account_for_off_pixels(gpu_ctx, oracle, sc, st, cam, spp, frame, ref, ok, label, limit=1e-4):
    """Every pixel of `frame` (the production kernel's) that is NOT within 1e-9 of the oracle's `ref` is accounted for, sample by sample: its
    samples are traced again one by one — by the device through the list probe (the render kernel's own code on an explicit (x, y, sample)
    list, vertex sequence recorded) and by the oracle — and
      (1) the production pixel is, bit for bit, the sequential sum of the device's per-sample values (src/trace.rs:203: nothing but samples went in),
      (2) the oracle's pixel is the sequential sum of the oracle's per-sample values,
      (3) every sample whose vertex sequence is the same on both sides agrees to 1e-9 relative OR 1e-12 absolute.  (Round 5 found what the second
          clause is for: 2 of the 265 M samples of the C2 frame keep their vertex sequence and differ by 1.8e-9 / 2.6e-9 relative — 7e-14 absolute:
          a grazing bounce whose weight carries a cosine n.l ~ 1e-7, so that the 1e-16 by which the device's sin / cos move the direction against
          the host libm's is 1e-9 of the cosine.  An absolute error of 1e-12 on radiances of order 1 is far inside the stated bar; a relative
          bar alone cannot hold for a quantity that passes through zero.)  So the pixel's difference beyond that is the sum over the samples
          whose vertex sequence DIFFERS (an ulp of libm turned a hit into a miss: a flipped sample), and
      (4) every off pixel holds a flipped sample or a grazing one (same sequence, outside 1e-9 relative, inside 1e-12 absolute).
    The number of off pixels is bounded by `limit` of the frame (the 1,000,000-sample campaign found 0 flipped samples: profiles/r04_parity_campaign.txt)
    and the counts are recorded (gpurun_out/off_pixels.jsonl on the GPU box -> profiles/)."""
    import json
    import os

    ys, xs = np.nonzero(~ok)
    n_off, n_px = len(ys), ok.size
    record = {"case": label, "pixels": int(n_px), "spp": int(spp), "off_pixels": int(n_off), "flipped_samples": 0, "max_flipped_per_off_pixel": 0,
              "grazing_samples": 0, "max_abs_diff_of_a_grazing_sample": 0.0, "max_rel_diff_of_a_grazing_sample": 0.0}
    assert n_off <= max(3, limit * n_px), "%s: %d of %d pixels are off" % (label, n_off, n_px)
    if n_off:
        xy = np.repeat(np.stack([xs, ys], axis=1), spp, axis=0).astype(np.uint32)
        smp = np.tile(np.arange(spp, dtype=np.uint32), n_off)
        ds = render.DeviceScene(gpu_ctx, sc)
        drgb, dpo, dps = probe.trace_samples(gpu_ctx, ds, cam, st, xy, smp, paths=True)
        ds.close()
        osc = oracle.OracleScene(sc)
        orgb = np.zeros_like(drgb)
        same_path = np.zeros(len(smp), dtype=bool)
        for i in range(len(smp)):
            rgb, po, ps = osc.trace_sample_path(cam, st, int(xy[i, 0]), int(xy[i, 1]), int(smp[i]))
            orgb[i] = rgb
            k = len(po)
            same_path[i] = (dpo[i, :k] == po).all() and (dps[i, :k] == ps).all() and (dpo[i, k:] == -2).all()
        drgb, orgb, same_path = drgb.reshape(n_off, spp, 3), orgb.reshape(n_off, spp, 3), same_path.reshape(n_off, spp)
        dsum, osum = np.zeros((n_off, 3)), np.zeros((n_off, 3))
        for k in range(spp):  # in sample order
            dsum, osum = dsum + drgb[:, k], osum + orgb[:, k]
        bits = lambda a, b: ((np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all()
        assert bits(frame[ys, xs], dsum), "%s: an off pixel is not the sum of its samples" % label  # (1)
        assert bits(ref[ys, xs], osum), "%s: the oracle's frame is not the sum of its samples" % label  # (2)
        absd = np.abs(drgb - orgb)
        within = rel_close(drgb, orgb, 1e-9) | (absd <= 1e-12)
        assert within[same_path].all(), "%s: a sample with the oracle's vertex sequence is off" % label  # (3)
        flipped = (~same_path).sum(axis=1)
        grazing = same_path & ~rel_close(drgb, orgb, 1e-9).all(axis=2)
        assert ((flipped >= 1) | grazing.any(axis=1)).all(), "%s: an off pixel with neither a flipped nor a grazing sample" % label  # (4)
        record["flipped_samples"], record["max_flipped_per_off_pixel"] = int(flipped.sum()), int(flipped.max())
        if grazing.any():
            scale = np.maximum(np.maximum(np.abs(drgb), np.abs(orgb)), 1e-300)
            record["grazing_samples"] = int(grazing.sum())
            record["max_abs_diff_of_a_grazing_sample"] = float(absd[grazing].max())
            record["max_rel_diff_of_a_grazing_sample"] = float((absd / scale)[grazing].max())
    print("off-pixel accounting: %s" % json.dumps(record))
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        if os.path.isdir(os.path.join(root, "gpurun_out")):
            with open(os.path.join(root, "gpurun_out", "off_pixels.jsonl"), "a") as f:
                f.write(json.dumps(record) + "\n")
    except OSError:
        pass
    return record


@pytest.mark.parametrize("config", ["C3", "C4", "C5"])
def test_spot_samples_against_the_oracle(gpu_ctx, oracle, dragon, config):
    """8,192 random (pixel, sample) pairs of the full-size configuration vs the oracle, hit sequence included."""
    st = scenes.config_settings(config)
    cam = st.camera_settings
    rng = np.random.default_rng(41)
    n = 8192
    # half of the pixels inside the mesh's footprint, half anywhere
    W, H = cam.backbuffer_width, cam.backbuffer_height
    xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], axis=1)
    xy[: n // 2, 0] = rng.integers(int(0.3 * W), int(0.7 * W), n // 2)
    xy[: n // 2, 1] = rng.integers(int(0.3 * H), int(0.85 * H), n // 2)
    xy = xy.astype(np.uint32)
    smp = rng.integers(0, st.sample_count, n).astype(np.uint32)
    ds, osc = render.DeviceScene(gpu_ctx, dragon), oracle.OracleScene(dragon)
    drgb, dpo, dps = probe.trace_samples(gpu_ctx, ds, cam, st, xy, smp, paths=True)
    ds.close()
    same = np.zeros(n, dtype=bool)
    orgb = np.zeros((n, 3))
    for i in range(n):
        rgb, po, ps = osc.trace_sample_path(cam, st, int(xy[i, 0]), int(xy[i, 1]), int(smp[i]))
        orgb[i] = rgb
        k = len(po)
        same[i] = (dpo[i, :k] == po).all() and (dps[i, :k] == ps).all() and (dpo[i, k:] == -2).all()
    assert same.mean() >= 0.999
    assert rel_close(drgb[same], orgb[same], 1e-9).all()
    assert (dpo == 1).any(axis=1).mean() > 0.25  # the mesh is on a good share of these paths


@pytest.mark.parametrize("config,spp,mode", [("C2", 128, "default"), ("C3", 16, "default"), ("C3", 16, "end"), ("C4", 16, "end"), ("C5", 8, "end")])
def test_spot_pixels_of_the_production_kernel_at_full_size(gpu_ctx, oracle, dragon, config, spp, mode):
    """Every BASELINE.json configuration at ITS OWN frame size through `rmd_render_tiles` — the production instantiation: persistent
    workgroups, a tile's samples split over several work items, pooled (pixel, sample) hand-out, per-sample scratch, ordered sum; asserted
    through rmd_last_launch_info — against the oracle: 320 spot pixels, all samples each, equal the oracle's sequential sums
    (src/trace.rs:203) to 1e-9.  "default" = rmd_settings.flags 0, the reference-identical mode (C2: zero-throughput paths ended, the scene
    has no grid; C3: traced on); "end" = RMD_RENDER_END_BLACK_PATHS, the opt-in that ends them on the mesh scenes too (C4 / C5 with flags 0
    are test_c4_shaped_launch and test_c5_thin_lens_at_full_size_in_tile_mode)."""
    st = scenes.config_settings(config, spp=spp)
    st.end_black_paths = mode == "end"
    cam = st.camera_settings
    W, H = cam.backbuffer_width, cam.backbuffer_height
    sc = scenes.reflective_spheres() if config == "C2" else dragon
    tiles = generate_tiles(W, H, st.tile_size)
    ds = render.DeviceScene(gpu_ctx, sc)
    fb = render.Framebuffer(gpu_ctx, W, H)
    render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb)
    info = gpu_ctx.last_launch_info()
    assert info.split_k > 1 and info.persistent == 1 and info.passes == 1, (info.split_k, info.persistent, info.passes)
    assert info.has_grid == (0 if config == "C2" else 1) and info.end_black_paths == (1 if config == "C2" or mode == "end" else 0)
    # the production form of each scene: mesh scenes keep their paths in queues, the spheres kernel has none
    assert info.buffered == 1 and info.queued == (0 if config == "C2" else 1), (info.buffered, info.queued)
    full = fb.download()
    fb.close(), ds.close()
    rng = np.random.default_rng(17)
    n = 320
    px = np.stack([rng.integers(int(0.25 * W), int(0.75 * W), n), rng.integers(int(0.25 * H), int(0.9 * H), n)], axis=1)
    px[: n // 4] = np.stack([rng.integers(0, W, n // 4), rng.integers(0, H, n // 4)], axis=1)
    xy = np.repeat(px, spp, axis=0).astype(np.uint32)
    smp = np.tile(np.arange(spp, dtype=np.uint32), n)
    o = oracle.OracleScene(sc).trace_samples(cam, st, xy, smp).reshape(n, spp, 3)
    acc = np.zeros((n, 3))
    for k in range(spp):
        acc = acc + o[:, k]  # in sample order
    got = full[px[:, 1], px[:, 0]]
    ok = rel_close(got, acc, 1e-9).all(axis=1)
    assert (acc > 0).any(axis=1).mean() > 0.5  # not a comparison of zeros
    # a pixel that is off is off by whole flipped samples (an ulp-level difference changing a hit sequence), each one found and counted
    ref = np.zeros_like(full)
    ref[px[:, 1], px[:, 0]] = acc
    mask = np.ones(full.shape[:2], dtype=bool)
    mask[px[:, 1], px[:, 0]] = ok
    rec = account_for_off_pixels(gpu_ctx, oracle, sc, st, cam, spp, full, ref, mask, "spot-pixels %s %d spp %s" % (config, spp, mode), limit=0.0)
    assert rec["off_pixels"] <= 3


@pytest.mark.parametrize("config,spp,mode", [("C2", 128, "default"), ("C3", 16, "default"), ("C3", 16, "end"), ("C4", 8, "default"), ("C5", 8, "default")])
def test_whole_frame_of_the_production_kernel_against_the_oracle(gpu_ctx, oracle, dragon, config, spp, mode):
    """EVERY pixel of a full-size frame (1920x1080; C4: 3840x2160, 8 bounces; C5: thin lens) rendered by the production instantiation (asserted through rmd_last_launch_info: persistent workgroups,
    samples split over several work items, pooled hand-out, ordered sum) against `oracle.render_tiles` — the reference's loop
    (src/trace.rs:197-205) on 16 host threads: every pixel within 1e-9 EXCEPT those — at most 1e-4 of the frame, counted and recorded — that
    account_for_off_pixels() shows to be off by flipped samples only; mean radiance equal to 1e-4.  C2: 265.4 M samples (the spheres kernel splits a tile's samples from 128 per pixel on), flags 0 (zero-throughput paths ended: the scene has
    no grid); C3: 33.2 M samples with flags 0 (every path traced) and with RMD_RENDER_END_BLACK_PATHS."""
    st = scenes.config_settings(config, spp=spp)
    st.end_black_paths = mode == "end"
    cam = st.camera_settings
    W, H = cam.backbuffer_width, cam.backbuffer_height
    sc = scenes.reflective_spheres() if config == "C2" else dragon
    tiles = generate_tiles(W, H, st.tile_size)
    ds = render.DeviceScene(gpu_ctx, sc)
    fb = render.Framebuffer(gpu_ctx, W, H)
    render.render_tiles(gpu_ctx, ds, cam, st, tiles, fb)
    info = gpu_ctx.last_launch_info()
    assert info.split_k > 1 and info.persistent == 1 and info.end_black_paths == (1 if config == "C2" or mode == "end" else 0)
    assert info.buffered == 1 and info.queued == (0 if config == "C2" else 1), (info.buffered, info.queued)
    dev = fb.download()
    fb.close(), ds.close()
    ref = oracle.OracleScene(sc, fast=True).render_tiles(cam, st, tiles, threads=16)
    ok = rel_close(dev, ref, 1e-9).all(axis=2)
    # no allowance for unexplained pixels: every pixel outside 1e-9 is re-traced sample by sample and must be off by flipped samples only
    account_for_off_pixels(gpu_ctx, oracle, sc, st, cam, spp, dev, ref, ok, "whole-frame %s %dx%d %d spp %s" % (config, W, H, spp, mode))
    assert abs(np.nanmean(dev) - np.nanmean(ref)) <= 1e-4 * np.nanmean(ref)
    assert (dev == ref).all(axis=2).mean() > 0.3  # a good share of the pixels is bit-identical, sums included


def test_full_frame_properties_1080p(gpu_ctx, dragon):
    """1920x1080, 2 spp on the mesh scene: (a) 8 round-robin tile shards sum to the full frame bit for bit (the 8-GPU
    reduce in miniature), (b) 1+1 spp in two launches == 2 spp in one, (c) every pixel finite and non-negative,
    (d) the ceiling strip reads exactly the emission."""
    st = scenes.config_settings("C3", spp=2)
    cam = st.camera_settings
    W, H = cam.backbuffer_width, cam.backbuffer_height
    tiles = generate_tiles(W, H, st.tile_size)
    assert len(tiles) == 2040
    ds = render.DeviceScene(gpu_ctx, dragon)
    full, part = render.Framebuffer(gpu_ctx, W, H), render.Framebuffer(gpu_ctx, W, H)
    render.render_tiles(gpu_ctx, ds, cam, st, tiles, full)
    ref = full.download()
    total = np.zeros_like(ref)
    for r in range(8):
        part.zero()
        render.render_tiles(gpu_ctx, ds, cam, st, tiles[r::8], part)
        total += part.download()
    assert total.tobytes() == ref.tobytes()
    part.zero()
    render.render_tiles(gpu_ctx, ds, cam, st, tiles, part, 0, 1)
    render.render_tiles(gpu_ctx, ds, cam, st, tiles, part, 1, 1)
    assert part.download().tobytes() == ref.tobytes()
    assert np.isfinite(ref).all() and (ref >= 0).all()
    assert (ref[0, W // 4 : 3 * W // 4] == 3.0).all()  # 2 samples x emission 1.5, seen directly
    # the mesh (metal, yellow: blue channel attenuated) is where the reference picture has the dragon
    centre = ref[int(0.45 * H) : int(0.75 * H), int(0.4 * W) : int(0.6 * W)]
    assert centre[..., 2].mean() < 0.5 * centre[..., 0].mean()
    full.close(), part.close(), ds.close()


def test_config2_frame_checksum_is_reproducible(gpu_ctx):
    """The headline workload's frame (ReflectiveSpheres 1080p) at 4 spp: two renders are bit-identical and the mean
    radiance matches the oracle's config-1 statistics (same scene, same integrator) to Monte-Carlo accuracy."""
    sc = scenes.reflective_spheres()
    st = scenes.config_settings("C2", spp=4)
    cam = st.camera_settings
    tiles = generate_tiles(1920, 1080, st.tile_size)
    ds = render.DeviceScene(gpu_ctx, sc)
    a, b = render.Framebuffer(gpu_ctx, 1920, 1080), render.Framebuffer(gpu_ctx, 1920, 1080)
    render.render_tiles(gpu_ctx, ds, cam, st, tiles, a)
    render.render_tiles(gpu_ctx, ds, cam, st, tiles, b)
    ia = a.download()
    assert ia.tobytes() == b.download().tobytes()
    assert 0.15 < ia.mean() / 4 < 0.30
    a.close(), b.close(), ds.close()


def test_rccl_entry_points_world_of_one(gpu_ctx):
    """rmd_comm_* / rmd_reduce_framebuffer through RCCL with a single rank: the reduce must leave the buffer untouched."""
    L = gpu_ctx.L
    uid = (C.c_uint8 * abi.RMD_COMM_ID_BYTES)()
    gpu_ctx.check(L.rmd_comm_unique_id(uid))
    assert any(uid)
    comm = C.c_void_p()
    gpu_ctx.check(L.rmd_comm_create(gpu_ctx.handle, uid, 0, 1, C.byref(comm)))
    fb = render.Framebuffer(gpu_ctx, 64, 32)
    data = np.random.default_rng(0).uniform(0, 1, (32, 64, 3))
    fb.upload(data)
    gpu_ctx.check(L.rmd_reduce_framebuffer(comm, fb.ptr, fb.n, 0))
    assert fb.download().tobytes() == data.tobytes()
    assert L.rmd_reduce_framebuffer(comm, fb.ptr, fb.n, 3) == abi.RMD_ERR_INVALID_ARGUMENT
    # the enqueue-only form (what lets a rank queue zeroing, render and reduce of several frames back to back): three frames queued, one wait
    st = Settings(scenes.camera(64, 32), sample_count=3, bounce_limit=3, seed=scenes.SEED)
    ds = render.DeviceScene(gpu_ctx, scenes.reflective_spheres())
    tiles = generate_tiles(64, 32, (32, 32))
    fb.zero()
    render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb)
    want = fb.download()
    for _ in range(3):
        fb.zero()
        render.render_tiles(gpu_ctx, ds, st.camera_settings, st, tiles, fb, sync=False)
        gpu_ctx.check(L.rmd_reduce_framebuffer_async(comm, fb.ptr, fb.n, 0))
    gpu_ctx.synchronize()
    assert fb.download().tobytes() == want.tobytes()
    assert L.rmd_reduce_framebuffer_async(comm, fb.ptr, fb.n, -1) == abi.RMD_ERR_INVALID_ARGUMENT
    ds.close()
    L.rmd_comm_destroy(comm)
    fb.close()


def test_torch_rccl_collectives_world_of_one():
    """bench.py's two ways of assembling the frame, through torch.distributed's nccl (= RCCL) backend on device tensors with a
    world of one — the only world RCCL accepts on a one-GPU box: the calls, tensor shapes and views are the ones an N-rank run makes.
    (In a child process: torch cannot initialise the GPU in a process that has loaded libraymond_hip.so's own ROCm runtime.)"""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import os, sys
sys.path.insert(0, %r)
import torch, torch.distributed as dist
from raymond_amd import shard
from raymond_amd.scene import generate_tiles
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29591")
dev = torch.device("cuda", 0); torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
W, H = 203, 117
tiles = generate_tiles(W, H, (32, 32))
fb = torch.rand(W * H * 3, dtype=torch.float64, device=dev)
want = fb.clone()
g = shard.OwnedTileGather(torch, W, H, tiles, 0, 1, dev, root=0)
g(dist, fb)
shard.reduce_framebuffer(dist, fb, root=0)
torch.cuda.synchronize()
assert torch.equal(fb, want)
assert g.pack(fb).shape == (W * H, 3)
dist.destroy_process_group()
print("collectives ok")
""" % root
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "collectives ok" in r.stdout, r.stderr[-2000:]


def test_gpu_grid_build_is_byte_identical_to_the_host_builder(gpu_ctx, oracle):
    """AccGrid::build_from_mesh on the GPU (atomics + scan + per-cell sort) == host builder == oracle."""
    from raymond_amd import lib
    from raymond_amd.scene import AccGrid, Mesh

    rng = np.random.default_rng(7)
    soup = Mesh((rng.uniform(-1, 1, size=(3000, 1, 3)) * np.array([1.0, 0.8, 0.5]) + rng.normal(scale=0.08, size=(3000, 3, 3))).reshape(-1, 9),
                rng.normal(size=(3000, 9)))
    meshes = [scenes.lumpy_sphere_mesh(13), scenes.lumpy_sphere_mesh(40), scenes.lumpy_sphere_mesh(91), soup]
    for m in meshes[:3]:
        m.bake_transform((0.0, -0.3, 2.9))
    for m in meshes:
        host, dev = AccGrid.build_from_mesh(m), AccGrid.build_from_mesh(m, ctx=gpu_ctx)
        assert np.array_equal(host.resolution, dev.resolution)
        assert host.bbox_min.tobytes() == dev.bbox_min.tobytes() and host.bbox_max.tobytes() == dev.bbox_max.tobytes()
        assert host.cell_size.tobytes() == dev.cell_size.tobytes()
        assert host.cells.tobytes() == dev.cells.tobytes()
        assert host.mapping_table.tobytes() == dev.mapping_table.tobytes()
    rc, og = oracle.grid_build(meshes[1])
    assert rc == 0 and og.mapping_table.tobytes() == AccGrid.build_from_mesh(meshes[1], ctx=gpu_ctx).mapping_table.tobytes()
    bad = scenes.lumpy_sphere_mesh(6, extent=(2.0, 0.5, 3.0))  # res.z > res.y: the reference's index quirk panics
    with pytest.raises(lib.RaymondError) as e:
        AccGrid.build_from_mesh(bad, ctx=gpu_ctx)
    assert e.value.status == abi.RMD_ERR_GRID_INDEX


def test_bench_contract_and_two_rank_rehearsal(gpu_ctx, tmp_path):
    """bench.py prints ONE JSON line with the driver's keys and, with --dump-outputs, writes the frame it timed; a 2-rank run
    (rehearsal mode: both ranks on this GPU, the collective over gloo — RCCL refuses two ranks on one device) assembles the same
    frame as the 1-rank run, bit for bit, by either route (gather of owned tiles, reduce of full frames)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--steps", "1", "--warmup", "1", "--spp", "24", "--no-cpu-baseline", "--no-roofline-leg"]
    dump = tmp_path / "outputs"
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--dump-outputs", str(dump)] + common, capture_output=True, text=True, timeout=300, cwd=root)
    assert one.returncode == 0, one.stderr[-2000:]
    lines = [l for l in one.stdout.split("\n") if l.strip()]
    assert len(lines) == 1
    a = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in a, key
    assert a["unit"] == "Msamples/s" and a["n_gpus"] == 1 and a["dtype"] == "f64" and a["vs_baseline"] is None and "workload" in a["config"]
    assert abs(a["value"] - 1920 * 1080 * 24 / (a["ms_per_step"] * 1e-3) / 1e6) < 1e-2 * a["value"]
    frame = np.load(dump / "framebuffer.npy")  # the last timed step's frame: sample sums, what rmd_render_tiles gives its caller
    assert frame.shape == (1080, 1920, 3) and frame.dtype == np.float64
    assert np.isclose(frame[np.isfinite(frame)].sum(), a["kernel"]["checksum"], rtol=1e-12, atol=0.0)
    # N > 1 without a launcher: bench.py starts its own ranks as fresh child processes (the form the driver uses at N = 1)
    env = dict(os.environ, RMD_BENCH_BACKEND="gloo")
    two = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"] + common, capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert two.returncode == 0, two.stderr[-2000:]
    b = json.loads([l for l in two.stdout.split("\n") if l.startswith("{")][0])
    assert b["n_gpus"] == 2 and b["scaling"] == "strong"
    assert b["kernel"]["checksum"] == a["kernel"]["checksum"]  # default: gather of the tiles each rank owns
    assert "gather" in b["config"]["workload"]
    # ... and under an explicit launcher, as the driver starts N > 1
    red = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29578", os.path.join(root, "bench.py"), "--gpus", "2", "--assemble", "reduce"] + common,
                         capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert red.returncode == 0, red.stderr[-2000:]
    c = json.loads([l for l in red.stdout.split("\n") if l.startswith("{")][0])
    assert c["kernel"]["checksum"] == a["kernel"]["checksum"]  # every pixel is non-zero on exactly one rank
    # the C-ABI's own collective (rmd_comm_* / rmd_reduce_framebuffer over RCCL) with the one rank RCCL accepts on a one-GPU box
    one_abi = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--assemble", "abi"] + common, capture_output=True, text=True, timeout=300, cwd=root)
    assert one_abi.returncode == 0, one_abi.stderr[-2000:]
    d = json.loads([l for l in one_abi.stdout.split("\n") if l.startswith("{")][0])
    assert d["kernel"]["checksum"] == a["kernel"]["checksum"]
    bad = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--assemble", "abi"] + common, capture_output=True, text=True, timeout=300, cwd=root, env=env)
    assert bad.returncode != 0  # two ranks on one device: refused loudly, no fallback


def _second_gpu_present(ctx):
    """Through the C-ABI itself: a context on device 1 exists exactly when the box has a second GPU."""
    h = C.c_void_p()
    status = ctx.L.rmd_context_create(1, C.byref(h))
    if status == abi.RMD_OK:
        ctx.L.rmd_context_destroy(h)
    return status == abi.RMD_OK


def test_two_gpus_over_rccl_by_every_route(gpu_ctx):
    """The N >= 2 path over the real thing — one rank per GPU, backend nccl = RCCL over xGMI — by all three ways of assembling the frame on
    rank 0 (gather of owned tiles, reduce of full frames through torch.distributed, reduce through the C-ABI's own rmd_comm_* /
    rmd_reduce_framebuffer_async): each must give the 1-GPU frame's checksum, and every rank must have seen a world of two on a device of its
    own.  Then the same through the C++ host mirror with two GPU workers.  Skipped, with the reason printed, on a box with one GPU (every
    one-GPU rehearsal of these routes runs over gloo or with a world of one: tests above)."""
    import json
    import os
    import subprocess
    import sys

    if not _second_gpu_present(gpu_ctx):
        pytest.skip("this box has one GPU: RCCL refuses two ranks on one device, so the N >= 2 routes over nccl cannot run here "
                    "(rehearsed over gloo in test_bench_contract_and_two_rank_rehearsal; this test runs by itself where rmd_context_create(1) succeeds)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--steps", "1", "--warmup", "1", "--spp", "24", "--no-cpu-baseline", "--no-roofline-leg"]
    env = dict(os.environ)
    env.pop("RMD_BENCH_BACKEND", None)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common, capture_output=True, text=True, timeout=300, cwd=root, env=env)
    assert one.returncode == 0, one.stderr[-2000:]
    a = json.loads([l for l in one.stdout.split("\n") if l.startswith("{")][0])
    for port, route in ((29581, "gather"), (29582, "reduce"), (29583, "abi")):
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                            "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--assemble", route] + common,
                           capture_output=True, text=True, timeout=600, cwd=root, env=env)
        assert r.returncode == 0, (route, r.stderr[-3000:])
        b = json.loads([l for l in r.stdout.split("\n") if l.startswith("{")][0])
        assert b["n_gpus"] == 2 and b["kernel"]["checksum"] == a["kernel"]["checksum"], route
        assert b["kernel"]["nonfinite_pixels"] == a["kernel"]["nonfinite_pixels"], route
        ranks = sorted(b["ranks"], key=lambda x: x["rank"])
        assert [x["rank"] for x in ranks] == [0, 1] and all(x["world_size_seen"] == 2 and x["backend"] == "nccl" for x in ranks), (route, ranks)
        assert sorted(x["device"] for x in ranks) == [0, 1], (route, ranks)  # one GPU each
        assert sum(x["samples_per_step"] for x in ranks) == 1920 * 1080 * 24 and all(x["samples_per_step"] > 0 for x in ranks), (route, ranks)
    # the C++ host mirror (raymond_amd/host: the stand-in for integration/gpu.rs) with one worker per GPU == one rmd_render_tiles call
    cli = os.path.join(root, "raymond_amd", "host", "raymond_cli")
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        W, H, spp, bounces = 96, 64, 7, 4
        raw, ppm = os.path.join(d, "o.f64"), os.path.join(d, "o.ppm")
        env2 = dict(env)
        env2.pop("RAYMOND_REHEARSE_ON_DEVICE0", None)
        r = subprocess.run([cli, "render", "dragon:12", str(W), str(H), str(spp), str(bounces), ppm, "--raw", raw, "--spi", "2", "--gpus", "2"],
                           capture_output=True, text=True, timeout=300, env=env2)
        assert r.returncode == 0, r.stderr[-2000:]
        img_cpp = np.fromfile(raw).reshape(H, W, 3)
    st = Settings(scenes.camera(W, H), sample_count=spp, tile_size=(32, 32), bounce_limit=bounces, seed=scenes.SEED)
    ds = render.DeviceScene(gpu_ctx, scenes.gold_dragon_standin(n=12))
    fb = render.Framebuffer(gpu_ctx, W, H)
    render.render_tiles(gpu_ctx, ds, st.camera_settings, st, generate_tiles(W, H, (32, 32)), fb)
    assert img_cpp.tobytes() == (fb.download() / float(spp)).tobytes()
    fb.close(), ds.close()
