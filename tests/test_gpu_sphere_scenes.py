"""Every launch form of the spheres kernel on the adversarial scenes of tests/sphere_scenes.py, on the GPU.

Per class and seed (and thin-lens variant) the same samples are rendered in eight forms into a framebuffer pre-filled with seeded non-zero values:

  A  RMD_TUNE_SAMPLE_SPLIT = 1                       the lane-per-path form (render_wave): buffered == 0
  B  split 0, the automatic launch                   the role-sorted form (render_wave_sorted): buffered == 1, has_grid == 0
  C  split 2, RMD_TUNE_LAUNCH_FORM = 1               persistent == 0, split_k == 2
  D  split 3, RMD_TUNE_LAUNCH_FORM = 2               split_k == 3; persistent == 1 unless the object table leaves no LDS for four waves' areas
                                                     (128 n + 4 x the wave's area > the budget, from rmd_probe_launch_sizes: more than 964
                                                     objects — the thousand-object rooms of table_edges — which then run one wave per work item)
  E  B, the scene created under RMD_TUNE_AXIS_PAIRS = 2   the axis rule without the generation trips' candidate sets
  F  B, the scene created under RMD_TUNE_AXIS_PAIRS = 1   every plane by the general test
  G  two launches over [0, 70) and [70, spp)
  H  B through rmd_render_tiles_moments              sums and squares against form A through rmd_render_tiles_moments

and every frame equals form A's BYTE FOR BYTE (`irregular`, whose samples may be NaN, with the suite's NaN-for-NaN comparison: same_bits of
tests/test_gpu_parity.py).  For shuffled_room, partial_room and fov_and_aspect forms A and B are rendered again over two rect lists off the
8-pixel lattice; the pixels no rect covers keep their pre-fill exactly.  Form B into a zeroed buffer agrees with the oracle's render at the
per-pixel bar of tests/test_gpu_fullsize.py: rel_close at 1e-9, and every pixel outside it accounted for sample by sample at
account_for_off_pixels' default limit (3 pixels on these frames).  In the DIAG build (RMD_DEBUG = 520) every generation trip of the non-lens
cases of five classes also runs the full visit: no cleared sphere registers a hit, no closest hit differs, while spheres and pairs ARE left out.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sphere_scenes as ss
from raymond_amd import abi, probe, render
from raymond_amd.scene import generate_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "raymond_amd", "csrc", "diag", "libraymond_hip.so")
CASES = ss.cases()
IDS = [ss.case_id(c) for c in CASES]
RECT_CASES = ss.cases(("shuffled_room", "partial_room", "fov_and_aspect"))
DIAG_CLASSES = ("shuffled_room", "partial_room", "camera_on_walls", "coincident_spheres", "fov_and_aspect")
FIRST_LAUNCH = 70  # form G: [0, 70) and [70, spp)


@pytest.fixture(scope="module")
def ctx(product_lib):
    """A context of this module's own: the tests change its tunables."""
    with render.Context(0) as c:
        yield c


def same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def equal_frames(name, a, b):
    if name == "irregular":  # a roughness-0 surface seen from behind: NaN samples, NaN for NaN
        from test_gpu_parity import same_bits

        return a.shape == b.shape and bool(same_bits(a, b).all())
    return same_bytes(a, b)


def prefill(case, W, H, salt=0):
    return np.random.default_rng([salt, case[1], int(case[2]), len(case[0])]).uniform(0.25, 3.0, (H, W, 3))


def persistent_expected(n_objects):
    """form D's launch is persistent while the object table leaves room for four waves' areas (render_kernel.hpp: the plan's lower end)"""
    s = probe.launch_sizes(probe.MODE_TILES_BUFFERED, False)
    return 1 if n_objects * s["object"] + 4 * s["wave"] <= s["budget"] else 0


class Forms:
    """One case's scene on the device and the eight ways to render its samples."""

    def __init__(self, ctx, case):
        self.ctx, self.case = ctx, case
        self.scene, self.cam, self.st, self.note = ss.build(case)
        self.W, self.H, self.spp = self.cam.backbuffer_width, self.cam.backbuffer_height, self.st.sample_count
        self.tiles = generate_tiles(self.W, self.H, self.st.tile_size)
        self.open = []

    def device_scene(self, axis_pairs=0):
        self.ctx.set_tunable(abi.RMD_TUNE_AXIS_PAIRS, axis_pairs)  # read when the scene is created
        try:
            ds = render.DeviceScene(self.ctx, self.scene)
        finally:
            self.ctx.set_tunable(abi.RMD_TUNE_AXIS_PAIRS, 0)
        self.open.append(ds)
        return ds

    def framebuffer(self):
        fb = render.Framebuffer(self.ctx, self.W, self.H)
        self.open.append(fb)
        return fb

    def close(self):
        for o in self.open:
            o.close()

    def render(self, ds, fb, base, split=0, form=0, ranges=None, tiles=None, fb_sq=None, base_sq=None):
        """-> (frame, squares or None, launch info of the last launch)"""
        self.ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, split), self.ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, form)
        try:
            fb.zero() if base is None else fb.upload(base)
            if fb_sq is not None:
                fb_sq.upload(base_sq)
            for begin, count in ranges or [(0, self.spp)]:
                render.render_tiles(self.ctx, ds, self.cam, self.st, self.tiles if tiles is None else tiles, fb, begin, count, framebuffer_sq=fb_sq)
            return fb.download(), (fb_sq.download() if fb_sq is not None else None), self.ctx.last_launch_info()
        finally:
            self.ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0), self.ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 0)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_launch_form_gives_form_a_byte_for_byte(ctx, case):
    name = case[0]
    f = Forms(ctx, case)
    try:
        base, base_sq = prefill(case, f.W, f.H), prefill(case, f.W, f.H, salt=1)
        ds, fb, fb_sq = f.device_scene(), f.framebuffer(), f.framebuffer()
        a, _, info = f.render(ds, fb, base, split=1)
        assert info.buffered == 0 and info.has_grid == 0, (info.buffered, info.split_k)
        assert (a != base).any() or (name == "one_lobe" and case[1] % 4 in (1, 2))  # (the two frames that are black by construction)
        frames = {}
        frames["B"], _, info = f.render(ds, fb, base)
        assert info.buffered == 1 and info.has_grid == 0, (info.buffered, info.split_k)
        frames["C"], _, info = f.render(ds, fb, base, split=2, form=1)
        assert info.buffered == 1 and info.persistent == 0 and info.split_k == 2, (info.persistent, info.split_k)
        frames["D"], _, info = f.render(ds, fb, base, split=3, form=2)
        assert info.buffered == 1 and info.split_k == 3 and info.persistent == persistent_expected(len(f.scene.objects)), (info.persistent, info.split_k)
        assert info.persistent == (0 if len(f.scene.objects) > 1000 else 1)  # (of these cases only the thousand-object rooms are past the LDS)
        for key, switch in (("E", 2), ("F", 1)):
            frames[key], _, info = f.render(f.device_scene(switch), fb, base)
            assert info.buffered == 1 and info.has_grid == 0
        frames["G"], _, _ = f.render(ds, fb, base, ranges=[(0, FIRST_LAUNCH), (FIRST_LAUNCH, f.spp - FIRST_LAUNCH)])
        a_sum, a_sq, info = f.render(ds, fb, base, split=1, fb_sq=fb_sq, base_sq=base_sq)
        assert info.buffered == 0
        frames["H"], h_sq, info = f.render(ds, fb, base, fb_sq=fb_sq, base_sq=base_sq)
        assert info.buffered == 1 and info.has_grid == 0
        for key, img in frames.items():
            diff = ~((img == a) | (np.isnan(img) & np.isnan(a)))
            print("%s form %s: %d of %d values differ from form A%s" % (ss.case_id(case), key, diff.sum(), a.size, "" if not diff.any() else
                  ", first at (y, x, c) %s: %r vs %r" % (tuple(np.argwhere(diff)[0]), img[tuple(np.argwhere(diff)[0])], a[tuple(np.argwhere(diff)[0])])))
        for key, img in frames.items():
            assert equal_frames(name, img, a), "%s: form %s differs from form A (%s)" % (ss.case_id(case), key, f.note)
        assert equal_frames(name, a_sum, a) and equal_frames(name, h_sq, a_sq), "%s: the moments' squares differ between forms A and B" % ss.case_id(case)
        assert (a_sq != base_sq).any() or (name == "one_lobe" and case[1] % 4 in (1, 2))
    finally:
        f.close()


def rect_lists(W, H):
    """Two rect lists off the 8-pixel lattice.  The first is test_degenerate_scenes_and_frames' [(5, 3, 3, 5), (20, 11, 17, 18)], made for its
    37x29 frame: cut to this frame (rmd_render_tiles refuses a rect that leaves it), and a rect that lies wholly outside a 97x9 or 9x97 frame
    moved to the frame's far corner at the same off-lattice offsets from it.  The second is a 7x5 tiling of the frame, every third tile left out."""
    first = []
    for (l, t, w, h) in ((5, 3, 3, 5), (20, 11, 17, 18)):
        if l >= W:
            l = max(W - 4, 0) | 1
        if t >= H:
            t = max(H - 4, 0) | 1
        first.append((l, t, min(w, W - l), min(h, H - t)))
    tiling = [(x, y, min(7, W - x), min(5, H - y)) for x in range(0, W, 7) for y in range(0, H, 5)]
    return first, [r for i, r in enumerate(tiling) if i % 3 != 2]


@pytest.mark.parametrize("case", RECT_CASES, ids=[ss.case_id(c) for c in RECT_CASES])
def test_rect_lists_off_the_lattice_in_both_forms(ctx, case):
    f = Forms(ctx, case)
    try:
        base = prefill(case, f.W, f.H, salt=2)
        ds, fb = f.device_scene(), f.framebuffer()
        for rects in rect_lists(f.W, f.H):
            assert all(w > 0 and h > 0 and l + w <= f.W and t + h <= f.H for (l, t, w, h) in rects)
            covered = np.zeros((f.H, f.W), dtype=bool)
            for (l, t, w, h) in rects:
                assert not covered[t : t + h, l : l + w].any()  # (rects do not overlap: a pixel's samples are added once)
                covered[t : t + h, l : l + w] = True
            assert covered.any() and not covered.all()
            a, _, info = f.render(ds, fb, base, split=1, tiles=rects)
            assert info.buffered == 0
            b, _, info = f.render(ds, fb, base, tiles=rects)
            assert info.buffered == 1 and info.has_grid == 0
            assert same_bytes(a, b), "%s: forms A and B differ over %s" % (ss.case_id(case), rects[:2])
            assert same_bytes(a[~covered], base[~covered]), "%s: a pixel no rect covers lost its pre-fill" % ss.case_id(case)
            assert (a[covered] != base[covered]).any()
    finally:
        f.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_role_sorted_form_agrees_with_the_oracle(ctx, oracle, case):
    from test_gpu_fullsize import account_for_off_pixels, rel_close  # the suite's per-pixel bar

    f = Forms(ctx, case)
    try:
        dev, _, info = f.render(f.device_scene(), f.framebuffer(), None)
        assert info.buffered == 1 and info.has_grid == 0
    finally:
        f.close()
    ref = oracle.OracleScene(f.scene).render_tiles(f.cam, f.st, f.tiles, threads=16)
    ok = rel_close(dev, ref, 1e-9).all(axis=2)
    account_for_off_pixels(ctx, oracle, f.scene, f.st, f.cam, f.spp, dev, ref, ok, "sphere scenes %s" % ss.case_id(case))


DIAG_CHILD = r"""
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import sphere_scenes as ss
from raymond_amd import lib, render
from raymond_amd.scene import generate_tiles

assert lib.LIB_PATH.endswith("diag/libraymond_hip.so"), lib.LIB_PATH
os.environ["RMD_DEBUG"] = "520"  # 8: event counters, 512: every generation trip ALSO runs the full visit and is compared with it
for case in ss.cases(%(classes)r, lens=False):
    scene, cam, st, note = ss.build(case)
    W, H = cam.backbuffer_width, cam.backbuffer_height
    with render.Context(0) as ctx:
        ds, fb = render.DeviceScene(ctx, scene), render.Framebuffer(ctx, W, H)
        sys.stderr.write("== %%s\n" %% ss.case_id(case)), sys.stderr.flush()
        render.render_tiles(ctx, ds, cam, st, generate_tiles(W, H, st.tile_size), fb)
        info = ctx.last_launch_info()
        assert info.buffered == 1 and info.has_grid == 0, case
        fb.close(), ds.close()
print("candidates ok")
"""


def test_the_full_visit_agrees_with_the_candidate_visit_on_the_classes_in_the_diag_build(product_lib):
    assert os.path.exists(DIAG_LIB), "build the DIAG library: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, RAYMOND_HIP_LIB=DIAG_LIB)
    env.pop("RMD_DEBUG", None)
    r = subprocess.run([sys.executable, "-c", DIAG_CHILD % {"root": ROOT, "classes": DIAG_CLASSES}], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "candidates ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    seen, name = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("== "):
            name = line[3:]
        m = re.search(r"primary candidates: lanes checked=(\d+) sphere turns left out=(\d+) trips with two axis pairs left out=(\d+) .*\(must be 0\)=(\d+) .*\(must be 0\)=(\d+)", line)
        if m and name:
            d = seen.setdefault(name, dict(lanes=0, turns=0, pair_trips=0, wrong=0, differs=0))
            for k, v in zip(("lanes", "turns", "pair_trips", "wrong", "differs"), m.groups()):
                d[k] += int(v)
    print(seen)
    cases = ss.cases(DIAG_CLASSES, lens=False)
    assert sorted(seen) == sorted(ss.case_id(c) for c in cases), r.stderr[-3000:]
    by_class = {c: dict(turns=0, pair_trips=0) for c in DIAG_CLASSES}
    for case in cases:
        d = seen[ss.case_id(case)]
        _, cam, st, _ = ss.build(case)
        assert d["wrong"] == 0 and d["differs"] == 0, (case, d)
        assert d["lanes"] == cam.backbuffer_width * cam.backbuffer_height * st.sample_count, (case, d)
        by_class[case[0]]["turns"] += d["turns"]
        by_class[case[0]]["pair_trips"] += d["pair_trips"]
    for c in DIAG_CLASSES:  # it ran, and it left objects out: every one of these classes drops spheres and pairs on the host probe too
        assert by_class[c]["turns"] > 0 and by_class[c]["pair_trips"] > 0, (c, by_class[c])
