"""Sweep of the spheres kernel's two-part work list on ONE GPU: kernel time of rank 0's share of an N-way C2 run for tail sizes and tail parts.
Needs the sweep build of the product library, whose contexts read RMD_WORK_LIST = "<tail tiles per wave slot, in halves>,<parts of a tail tile>"
(0 halves = no whole items: the uniform split):

    make -C raymond_amd/csrc OUT=sweep EXTRA=-DRMD_WORK_LIST_SWEEP=1 sweep/libraymond_hip.so
    RAYMOND_HIP_LIB=raymond_amd/csrc/sweep/libraymond_hip.so python tools/work_list_sweep.py [spp] [N,N,...] [halves,...] [parts,...] [frames]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import lib, render, scenes, shard
from raymond_amd.scene import generate_tiles

assert "sweep" in lib.LIB_PATH, "set RAYMOND_HIP_LIB to the sweep build (see above): %s ignores RMD_WORK_LIST" % lib.LIB_PATH
spp = int(sys.argv[1]) if len(sys.argv) > 1 else 500
ns = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1]
halves = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [0, 2, 3, 4, 6]
parts = [int(v) for v in sys.argv[4].split(",")] if len(sys.argv) > 4 else [4, 5, 6, 7]
frames = int(sys.argv[5]) if len(sys.argv) > 5 else 7
st = scenes.config_settings("C2", spp=spp)
cam = st.camera_settings
sc = scenes.reflective_spheres()
tiles = generate_tiles(cam.backbuffer_width, cam.backbuffer_height, st.tile_size)
for n in ns:
    share = shard.shard_tiles(tiles, 0, n)
    for h in halves:
        for p in parts if h else parts[:1]:
            os.environ["RMD_WORK_LIST"] = "%d,%d" % (h, p)  # read when the context is created
            with render.Context(0) as ctx:
                ds = render.DeviceScene(ctx, sc)
                fb = render.Framebuffer(ctx, cam.backbuffer_width, cam.backbuffer_height)
                ms = []
                for _ in range(frames + 1):
                    fb.zero()
                    render.render_tiles(ctx, ds, cam, st, share, fb)
                    ms.append(ctx.last_kernel_ms())
                ms = ms[1:]  # (the first frame allocates the scratch)
                info = ctx.last_launch_info()
                print("C2 %d spp N=%d tail %.1f tiles/slot parts %d (split_k %d): min %.3f median %.3f max %.3f ms" % (
                    spp, n, h / 2, p, info.split_k, min(ms), statistics.median(ms), max(ms)), flush=True)
                fb.close(), ds.close()
