"""Every launch form of the spheres kernel on the adversarial scenes of tests/sphere_scenes.py, on the GPU.

Per class and seed (and thin-lens variant) the same samples are rendered in eleven forms into a framebuffer pre-filled with seeded non-zero values:

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
  I  B, the scene created under RMD_TUNE_AXIS_PAIRS = 3   the candidate sets without the tile classes: every work item general
  J  RMD_TUNE_SPLIT_MIN_SAMPLES = 1                  64 items a wave tile, of two or three samples: shorter than a BLACK item's generation round
  K  RMD_TUNE_SCRATCH_CAP_MB = 1                     several passes (rmd_last_launch_info: at least 2 where the frame's samples exceed 1 MiB)

and every frame equals form A's BYTE FOR BYTE (`irregular`, whose samples may be NaN, with the suite's NaN-for-NaN comparison: same_bits of
tests/test_gpu_parity.py).  Form A is the lane-per-path kernel, which has no tile classes: for the five classes aimed at them
(ss.TILE_CLASS_CLASSES) this is what holds an EMITTER and a BLACK item's code to code that is not its own.  For shuffled_room, partial_room,
fov_and_aspect, one_wall_mixed and ragged_one_wall forms A and B are rendered again over two rect lists off the 8-pixel lattice; the pixels
no rect covers keep their pre-fill exactly.  The tile-class classes are also rendered in forms A, B and I into a pre-fill of signed zeros,
denormals and 1e300 (a classed item's zero and an emitter's -0.0 must ADD as form A's do), and three of their cases at sample counts around the
round size: 2 .. 129 samples per pixel in form J, 8, 9 and 130 from sample 7 on in forced splits of 2 and 3.  Form B into a zeroed buffer
agrees with the oracle's render at the per-pixel bar of tests/test_gpu_fullsize.py: rel_close at 1e-9, and every pixel outside it accounted
for sample by sample at account_for_off_pixels' default limit (3 pixels on these frames).  In the DIAG build (RMD_DEBUG = 520) every generation trip of the non-lens
cases of five classes also runs the full visit: no cleared sphere registers a hit, no closest hit differs, while spheres and pairs ARE left out.
With RMD_DEBUG = 1544 the non-lens cases of one_wall_mixed, black_walls, emitter_colours and ragged_one_wall run every class-ended sample's full path
beside it: none disagrees, the items' classes are the host probe's, the rounds are cut where every tile is BLACK, and where the whole frame is
BLACK the samples ended in pass A and the survivors are the frame's samples.
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
# (ragged_one_wall's 1x1 frame has no pixel a rect list could leave out)
RECT_CASES = [c for c in ss.cases(("shuffled_room", "partial_room", "fov_and_aspect", "one_wall_mixed", "ragged_one_wall")) if c[:2] != ("ragged_one_wall", 0)]
NEW_CASES = ss.cases(ss.TILE_CLASS_CLASSES)  # the classes aimed at the tile classes
ROUND_CASES = (("black_walls", 1, False), ("emitter_colours", 1, False), ("one_wall_mixed", 0, False))  # BLACK-heavy, EMITTER-heavy, and all three kinds at bounce limit 1
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

    def render(self, ds, fb, base, split=0, form=0, ranges=None, tiles=None, fb_sq=None, base_sq=None, min_samples=0, cap_mb=0):
        """-> (frame, squares or None, launch info of the last launch)"""
        self.ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, split), self.ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, form)
        self.ctx.set_tunable(abi.RMD_TUNE_SPLIT_MIN_SAMPLES, min_samples), self.ctx.set_tunable(abi.RMD_TUNE_SCRATCH_CAP_MB, cap_mb)
        try:
            fb.zero() if base is None else fb.upload(base)
            if fb_sq is not None:
                fb_sq.upload(base_sq)
            for begin, count in ranges or [(0, self.spp)]:
                render.render_tiles(self.ctx, ds, self.cam, self.st, self.tiles if tiles is None else tiles, fb, begin, count, framebuffer_sq=fb_sq)
            return fb.download(), (fb_sq.download() if fb_sq is not None else None), self.ctx.last_launch_info()
        finally:
            self.ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0), self.ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 0)
            self.ctx.set_tunable(abi.RMD_TUNE_SPLIT_MIN_SAMPLES, 0), self.ctx.set_tunable(abi.RMD_TUNE_SCRATCH_CAP_MB, 0)

    def scratch_bytes(self):
        """what the frame's samples take in the split launches' scratch: 32 bytes a sample, 64 lanes a wave tile (api.cpp: bytes_per_sample)"""
        n_wave_tiles = sum(-(-int(w) // 8) * -(-int(h) // 8) for (_, _, w, h) in self.tiles)
        return n_wave_tiles * 64 * 32 * self.spp


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
        for key, switch in (("E", 2), ("F", 1), ("I", 3)):
            frames[key], _, info = f.render(f.device_scene(switch), fb, base)
            assert info.buffered == 1 and info.has_grid == 0
        frames["G"], _, _ = f.render(ds, fb, base, ranges=[(0, FIRST_LAUNCH), (FIRST_LAUNCH, f.spp - FIRST_LAUNCH)])
        frames["J"], _, info = f.render(ds, fb, base, min_samples=1)
        assert info.buffered == 1 and info.has_grid == 0 and info.split_k == min(f.spp, 64), (info.buffered, info.split_k)
        frames["K"], _, info = f.render(ds, fb, base, cap_mb=1)
        assert info.buffered == 1 and info.has_grid == 0
        print("%s form K: %d passes for %d bytes of samples" % (ss.case_id(case), info.passes, f.scratch_bytes()))
        if f.scratch_bytes() > 1 << 20:
            assert info.passes >= 2, (info.passes, f.scratch_bytes())
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
    moved to the frame's far corner at the same off-lattice offsets from it.  The second is a 7x5 tiling of the frame, every third tile left out.
    In the frames of a few pixels (ragged_one_wall: one pixel wide, 9x9): a moved rect that still leaves the frame starts at its last pixel, one
    that would overlap an earlier rect is left out, and a tiling of fewer than three tiles leaves out its last."""
    first = []
    for (l, t, w, h) in ((5, 3, 3, 5), (20, 11, 17, 18)):
        if l >= W:
            l = min(max(W - 4, 0) | 1, W - 1)
        if t >= H:
            t = min(max(H - 4, 0) | 1, H - 1)
        w, h = min(w, W - l), min(h, H - t)
        if not any(l < l2 + w2 and l2 < l + w and t < t2 + h2 and t2 < t + h for (l2, t2, w2, h2) in first):
            first.append((l, t, w, h))
    tiling = [(x, y, min(7, W - x), min(5, H - y)) for x in range(0, W, 7) for y in range(0, H, 5)]
    return first, [r for i, r in enumerate(tiling) if i % 3 != 2] if len(tiling) >= 3 else tiling[:-1]


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
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(dev == ref, 0.0, np.abs(dev - ref) / np.maximum(np.maximum(np.abs(dev), np.abs(ref)), 1e-300))
    print("%s: worst relative difference from the oracle %.3g, %d of %d pixels outside 1e-9" % (ss.case_id(case), np.nanmax(rel, initial=0.0), (~ok).sum(), ok.size))
    account_for_off_pixels(ctx, oracle, f.scene, f.st, f.cam, f.spp, dev, ref, ok, "sphere scenes %s" % ss.case_id(case))


def special_prefill(case, W, H):
    """a framebuffer of -0.0, +0.0, denormals of both signs, 1e300 and ordinary values, seeded"""
    rng = np.random.default_rng([3, case[1], int(case[2]), len(case[0])])
    special = np.array([-0.0, 0.0, 5e-324, -5e-324, 2.0**-1030, 1e300, -1e300])
    pick = rng.integers(0, 2 * len(special), (H, W, 3))  # half of the values special, half ordinary
    return np.where(pick < len(special), special[pick % len(special)], rng.uniform(-2.0, 3.0, (H, W, 3)))


@pytest.mark.parametrize("case", NEW_CASES, ids=[ss.case_id(c) for c in NEW_CASES])
def test_classed_items_add_into_signed_zeros_denormals_and_huge_values_as_form_a_does(ctx, case):
    """The kernel's zero for an ended sample and an emitter's -0.0 or denormal are ADDED to what the pixel holds: -0.0 + 0.0, -0.0 + -0.0, a
    denormal + a denormal, 1e300 + 1e150 must come out of a classed item (B), of a general item (I: the candidate sets without the classes) and of
    the lane-per-path kernel (A) with the same bytes."""
    f = Forms(ctx, case)
    try:
        base = special_prefill(case, f.W, f.H)
        assert (np.signbit(base) & (base == 0.0)).any() or base.size < 16
        ds, fb = f.device_scene(), f.framebuffer()
        a, _, info = f.render(ds, fb, base, split=1)
        assert info.buffered == 0 and np.isfinite(a).all()
        b, _, info = f.render(ds, fb, base)
        assert info.buffered == 1 and info.has_grid == 0
        i, _, info = f.render(f.device_scene(3), fb, base)
        assert info.buffered == 1 and info.has_grid == 0
        for key, img in (("B", b), ("I", i)):
            print("%s form %s: %d of %d values differ from form A" % (ss.case_id(case), key, (img.view(np.uint64) != a.view(np.uint64)).sum(), a.size))
        assert same_bytes(b, a) and same_bytes(i, a), "%s: forms A, B and I differ over a pre-fill of signed zeros, denormals and 1e300" % ss.case_id(case)
    finally:
        f.close()


@pytest.mark.parametrize("case", ROUND_CASES, ids=[ss.case_id(c) for c in ROUND_CASES])
def test_sample_counts_around_the_round_size_give_form_a(ctx, case):
    """A generation round takes up to 128 (pixel, sample) pairs: items of 1 .. 3 samples (form J: RMD_TUNE_SPLIT_MIN_SAMPLES = 1) at 2 .. 129 samples
    per pixel, and forced splits in two and three at 8, 9 and 130 samples from sample 7 on.  Every frame against form A over the same samples."""
    f = Forms(ctx, case)
    try:
        base = prefill(case, f.W, f.H, salt=4)
        ds, fb = f.device_scene(), f.framebuffer()
        _, cls, _ = probe.tile_classes(f.cam, f.st, f.scene, np.array([(x, y, min(8, f.W - x), min(8, f.H - y)) for x in range(0, f.W, 8) for y in range(0, f.H, 8)], dtype=np.uint32))
        assert (cls != probe.TILE_GENERAL).any()
        a_of = {}

        def form_a(begin, n):
            if (begin, n) not in a_of:
                a_of[(begin, n)], _, info = f.render(ds, fb, base, split=1, ranges=[(begin, n)])
                assert info.buffered == 0
            return a_of[(begin, n)]

        for n in (2, 3, 63, 64, 65, 127, 129):
            j, _, info = f.render(ds, fb, base, min_samples=1, ranges=[(0, n)])
            assert info.buffered == 1 and info.has_grid == 0 and info.split_k == min(n, 64), (n, info.buffered, info.split_k)
            assert same_bytes(j, form_a(0, n)), "%s: form J differs from form A at %d samples per pixel" % (ss.case_id(case), n)
        for n in (8, 9, 130):
            for k in (2, 3):
                got, _, info = f.render(ds, fb, base, split=k, ranges=[(7, n)])
                assert info.buffered == 1 and info.split_k == min(k, n // 4), (n, k, info.buffered, info.split_k)
                assert same_bytes(got, form_a(7, n)), "%s: a split in %d differs from form A at samples [7, %d)" % (ss.case_id(case), k, 7 + n)
    finally:
        f.close()


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


CLASS_DIAG_CLASSES = ("one_wall_mixed", "black_walls", "emitter_colours", "ragged_one_wall")
CLASS_DIAG_CHILD = r"""
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import sphere_scenes as ss
from raymond_amd import abi, lib, render
from raymond_amd.scene import generate_tiles

assert lib.LIB_PATH.endswith("diag/libraymond_hip.so"), lib.LIB_PATH
# 8: event counters, 512: every sample a class ends has its full path run beside it, 1024: the work list's tail is 4 wave tiles (whole items too)
os.environ["RMD_DEBUG"] = "1544"
with render.Context(0) as ctx:
    ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 2)  # persistent, however few the items
    for case in ss.cases(%(classes)r, lens=False):
        scene, cam, st, note = ss.build(case)
        W, H = cam.backbuffer_width, cam.backbuffer_height
        ds, fb = render.DeviceScene(ctx, scene), render.Framebuffer(ctx, W, H)
        sys.stderr.write("== %%s\n" %% ss.case_id(case)), sys.stderr.flush()
        render.render_tiles(ctx, ds, cam, st, generate_tiles(W, H, st.tile_size), fb)
        info = ctx.last_launch_info()
        assert info.buffered == 1 and info.has_grid == 0 and info.passes == 1, case
        fb.close(), ds.close()
print("tile classes ok")
"""


def test_classed_items_of_the_new_classes_agree_with_their_full_path_in_the_diag_build(product_lib):
    """RMD_DEBUG = 1544 over the non-lens cases of four classes, the classes on: every sample a class ends without a ray has its full path run
    beside it, every generation trip the full visit.  Nothing disagrees; the rounds ARE cut where every tile is BLACK; the items' classes are the
    host probe's."""
    from test_gpu_tile_classes import CLASS_KEYS, CLASS_LINE

    assert os.path.exists(DIAG_LIB), "build the DIAG library: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, RAYMOND_HIP_LIB=DIAG_LIB)
    env.pop("RMD_DEBUG", None)
    r = subprocess.run([sys.executable, "-c", CLASS_DIAG_CHILD % {"root": ROOT, "classes": CLASS_DIAG_CLASSES}], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "tile classes ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    seen, name = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("== "):
            name = line[3:]
        m = re.search(CLASS_LINE, line)
        if m and name:
            d = seen.setdefault(name, dict.fromkeys(CLASS_KEYS + ("wrong", "differs", "lines"), 0))
            d["lines"] += 1
            for k, v in zip(CLASS_KEYS, m.groups()):
                d[k] += int(v)
        m = re.search(r"primary candidates: .*\(must be 0\)=(\d+) .*\(must be 0\)=(\d+)", line)
        if m and name:
            d = seen.setdefault(name, dict.fromkeys(CLASS_KEYS + ("wrong", "differs", "lines"), 0))
            d["wrong"] += int(m.group(1))
            d["differs"] += int(m.group(2))
    cases = ss.cases(CLASS_DIAG_CLASSES, lens=False)
    assert sorted(seen) == sorted(ss.case_id(c) for c in cases), r.stderr[-3000:]
    cut = dict.fromkeys(CLASS_DIAG_CLASSES, 0)
    for case in cases:
        d = seen[ss.case_id(case)]
        print(ss.case_id(case), d)
        scene, cam, st, _ = ss.build(case)
        W, H = cam.backbuffer_width, cam.backbuffer_height
        tiles = np.array([(x, y, min(8, W - x), min(8, H - y)) for x in range(0, W, 8) for y in range(0, H, 8)], dtype=np.uint32)
        on, cls, _ = probe.tile_classes(cam, st, scene, tiles)
        assert on and d["lines"] == 1, (case, d)
        assert d["bad_samples"] == 0 and d["bad_rays"] == 0 and d["wrong"] == 0 and d["differs"] == 0, (case, d)
        for key, c in (("general", probe.TILE_GENERAL), ("emitter", probe.TILE_EMITTER), ("black", probe.TILE_BLACK)):
            assert (d[key] > 0) == bool((cls == c).any()), (case, key, d)  # an item's class is its tile's
        if (cls == probe.TILE_BLACK).any():
            assert d["rounds"] > 0 and d["ended"] > 0 and d["survivors"] > 0 and d["checked"] >= d["ended"], (case, d)
        if (cls == probe.TILE_BLACK).all():  # every (pixel, sample) pair of the frame went through a round: ended in pass A, or a survivor
            assert d["ended"] + d["survivors"] == W * H * st.sample_count and d["checked"] == d["ended"], (case, d)
        if (cls == probe.TILE_EMITTER).all():
            assert d["checked"] == W * H * st.sample_count and d["rounds"] == 0, (case, d)
        cut[case[0]] += d["cut"]
    assert cut["black_walls"] > 0 and cut["emitter_colours"] == 0, cut  # rounds of more than 64 survivors occurred, and were cut
