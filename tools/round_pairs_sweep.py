"""Sweep of the round size of the spheres kernel's BLACK items (render_kernel.hpp: kRoundPairs) on ONE GPU: kernel time of the C2 frame and the
frame's SHA-256 for each build — the frame must be the same for every N.  Needs one build of the product library per N:

    for n in 96 104 112 120; do make -C raymond_amd/csrc OUT=round$n EXTRA=-DRMD_ROUND_PAIRS=$n round$n/libraymond_hip.so; done
    python tools/round_pairs_sweep.py [N,N,...] [spp] [frames] [passes]

(N = 128 is the library as shipped.)  Every build runs in a process of its own, under a time limit; the first that fails ends the sweep."""
import hashlib
import os
import statistics
import subprocess
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)

if len(sys.argv) > 1 and sys.argv[1] == "--child":
    from raymond_amd import render, scenes
    from raymond_amd.scene import generate_tiles

    n, spp, frames = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    st = scenes.config_settings("C2", spp=spp)
    cam = st.camera_settings
    tiles = generate_tiles(cam.backbuffer_width, cam.backbuffer_height, st.tile_size)
    with render.Context(0) as ctx:
        ds = render.DeviceScene(ctx, scenes.reflective_spheres())
        fb = render.Framebuffer(ctx, cam.backbuffer_width, cam.backbuffer_height)
        ms = []
        for _ in range(frames + 1):
            fb.zero()
            render.render_tiles(ctx, ds, cam, st, tiles, fb)
            ms.append(ctx.last_kernel_ms())
        ms = ms[1:]  # (the first frame allocates the scratch)
        digest = hashlib.sha256(fb.download().tobytes()).hexdigest()[:16]
        print("N=%s C2 %d spp: min %.3f median %.3f max %.3f ms, frame %s" % (n, spp, min(ms), statistics.median(ms), max(ms), digest), flush=True)
        fb.close(), ds.close()
    sys.exit(0)

ns = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [96, 104, 112, 120, 128]
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 500
frames = int(sys.argv[3]) if len(sys.argv) > 3 else 7
passes = int(sys.argv[4]) if len(sys.argv) > 4 else 2
for _ in range(passes):
    for n in ns:
        lib = os.path.join(root, "raymond_amd", "csrc", "libraymond_hip.so" if n == 128 else "round%d/libraymond_hip.so" % n)
        assert os.path.exists(lib), "build it first (see above): %s" % lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(spp), str(frames)], env=dict(os.environ, RAYMOND_HIP_LIB=lib), timeout=300)
        if r.returncode != 0:
            sys.exit("N=%d: the run failed (status %d); the sweep ends here" % (n, r.returncode))
