"""Kernel time of the library's own (automatic) launch for a list of workloads and N-way tile shares, for whichever library RAYMOND_HIP_LIB
names — run once per build to compare two builds:  python tools/auto_launch_times.py TAG [WORKLOAD[-trace]:N,...]
(default C2:1,C2:2,C2:8,C2-trace:1,C3:1 at 500 spp; rank 0's share of an N-way run; min / median / max of the launches after the first)"""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import lib, render, scenes, shard
from raymond_amd.scene import generate_tiles
tag = sys.argv[1]
what = sys.argv[2].split(",") if len(sys.argv) > 2 else ["C2:1", "C2:2", "C2:8", "C2-trace:1", "C3:1"]
with render.Context(0) as ctx:
    for w in what:
        arg, n = w.split(":"); n = int(n)
        name, _, mode = arg.partition("-")
        st = scenes.config_settings(name, spp=500)
        st.trace_black_paths = mode == "trace"
        cam = st.camera_settings
        sc = getattr(scenes, scenes.CONFIGS[name][0])()
        tiles = shard.shard_tiles(generate_tiles(cam.backbuffer_width, cam.backbuffer_height, st.tile_size), 0, n)
        ds = render.DeviceScene(ctx, sc); fb = render.Framebuffer(ctx, cam.backbuffer_width, cam.backbuffer_height)
        ms = []
        for _ in range(4 if name == "C3" else 8):
            fb.zero(); render.render_tiles(ctx, ds, cam, st, tiles, fb); ms.append(ctx.last_kernel_ms())
        ms = ms[1:]
        info = ctx.last_launch_info()
        print("%s %s N=%d split_k %d: min %.3f median %.3f max %.3f ms" % (tag, arg, n, info.split_k, min(ms), statistics.median(ms), max(ms)), flush=True)
        fb.close(); ds.close()
