"""Every launch form of the mesh kernel on the adversarial scenes of tests/mesh_scenes.py, on the GPU.

Per class and seed (and thin-lens variant; `materials` also under RMD_RENDER_TRACE_BLACK_PATHS and RMD_RENDER_END_BLACK_PATHS) the same samples are
rendered into a framebuffer pre-filled with seeded non-zero values, in these forms (FORMS below; what rmd_last_launch_info must report beside each):

  A   RMD_TUNE_PATH_QUEUES 1, SAMPLE_SPLIT 1, LAUNCH_FORM 0       direct, lane per path: buffered == 0, queued == 0, has_grid == 1
  B   LAUNCH_FORM 2                                               render_wave_queued: queued == 1, persistent == 1, buffered == 1, chained == 0
  C   B with SAMPLE_SPLIT 5, and with SAMPLE_SPLIT 12             queued == 1, split_k == 5 / 12 (12 items of 4 samples a wave tile: an item's 256
                                                                  (pixel, sample) pairs are the 256 entries of a queue — launch.hpp: kQueuePaths)
  D   B with SCRATCH_CAP_MB 1                                     queued == 1, passes >= 2
  E   B with WALK_CUT 1 (no walk put aside), and with WALK_CUT 13 queued == 1
  F   PATH_QUEUES 1, CHAIN_ITEMS 2, LAUNCH_FORM 2                 render_wave<.., CHAIN>: chained == 1, queued == 0
  G   SAMPLE_SPLIT 3, LAUNCH_FORM 1                               one wave per item: persistent == 0
  H   every tunable 0                                             the library's own choice: recorded, not asserted
  I   B, the scene created under RMD_TUNE_AXIS_PAIRS = 1 (every plane by the general test), and under RMD_TUNE_MASK_BUDGET = 256: queued == 1
  J   B as two launches over [0, 20) and [20, 48)
  K   B, and A, with WALK_BATCH 1 and 1000
  L   A and B through rmd_render_tiles_moments: sums and squares; the moments launch takes the form the plain launch took

and every frame equals form A's BYTE FOR BYTE (the classes of mesh_scenes.NAN_FOR_NAN, whose samples may be NaN, with the suite's NaN-for-NaN
comparison: same_bits of tests/test_gpu_parity.py).  Form A changed the pre-fill in every case: no case is black by construction.  What
rmd_scene_create decided for the case — n_grid_objects, n_grids, grid_mask, visit_mask, axis_pairs, walk_steps_bound, every grid's mask_shift — is
read back through rmd_probe_scene_plan and asserted to be what the class names.  For shared_grid, every_ray_walks and partial_room_with_mesh forms A
and B are rendered again over the two off-lattice rect lists of tests/test_gpu_sphere_scenes.py; the pixels no rect covers keep their pre-fill
exactly.  Form B into a zeroed buffer, flags 0, agrees with the oracle's render at the per-pixel bar of tests/test_gpu_fullsize.py: rel_close at
1e-9, every pixel outside it accounted for sample by sample at account_for_off_pixels' default limit (3 pixels on these frames).  An
RMD_RENDER_END_BLACK_PATHS frame differs from the flags-0 frame only where that one is non-finite.  In the DIAG build (RMD_DEBUG = 72: event
counters and the pre-test cross-check) form B of the non-lens cases of five classes drops no pair that passes the reference's test, puts walks aside
with one grid object and never with two or three, holds and pushes rays where every ray walks and neither where no ray enters a box.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mesh_scenes as ms
import sphere_scenes as ss
from raymond_amd import abi, probe, render
from raymond_amd.scene import generate_tiles
from test_gpu_sphere_scenes import rect_lists

pytestmark = pytest.mark.gpu

T = abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "raymond_amd", "csrc", "diag", "libraymond_hip.so")
CASES = ms.cases()
IDS = [ms.case_id(c) for c in CASES]
MODES = [(c, i) for c in CASES for i in range(1 + len(ms.render_flags(c)))]  # (case, 0 = flags 0, else the i-th of render_flags)
MODE_IDS = [ms.case_id(c) + ("" if i == 0 else "-" + "-".join(ms.render_flags(c)[i - 1])) for c, i in MODES]
RECT_CASES = ms.cases(("shared_grid", "every_ray_walks", "partial_room_with_mesh"))
DIAG_CLASSES = ("shared_grid", "three_grids", "no_ray_enters", "every_ray_walks", "mirror_box")
FIRST_LAUNCH = 20  # form J: [0, 20) and [20, spp)
KEYS = (T.RMD_TUNE_SAMPLE_SPLIT, T.RMD_TUNE_WALK_BATCH, T.RMD_TUNE_MASK_BUDGET, T.RMD_TUNE_LAUNCH_FORM, T.RMD_TUNE_SCRATCH_CAP_MB, T.RMD_TUNE_WALK_CUT,
        T.RMD_TUNE_SPLIT_MIN_SAMPLES, T.RMD_TUNE_CHAIN_ITEMS, T.RMD_TUNE_AXIS_PAIRS, T.RMD_TUNE_PATH_QUEUES)
A = {T.RMD_TUNE_PATH_QUEUES: 1, T.RMD_TUNE_SAMPLE_SPLIT: 1, T.RMD_TUNE_LAUNCH_FORM: 0}
B = {T.RMD_TUNE_LAUNCH_FORM: 2}
INFO_FIELDS = ("passes", "split_k", "persistent", "end_black_paths", "has_grid", "waves_per_workgroup", "buffered", "chained", "queued")
# name -> (render tunables, tunables the scene is created under, what the launch info must hold)
FORMS = {
    "B": (B, {}, dict(queued=1, persistent=1, buffered=1, chained=0, has_grid=1)),
    "C": ({**B, T.RMD_TUNE_SAMPLE_SPLIT: 5}, {}, dict(queued=1, split_k=5)),
    "C-256-pairs": ({**B, T.RMD_TUNE_SAMPLE_SPLIT: 12}, {}, dict(queued=1, split_k=12)),
    "D": ({**B, T.RMD_TUNE_SCRATCH_CAP_MB: 1}, {}, dict(queued=1)),
    "E-no-walk-cut": ({**B, T.RMD_TUNE_WALK_CUT: 1}, {}, dict(queued=1)),
    "E-cut-of-12": ({**B, T.RMD_TUNE_WALK_CUT: 13}, {}, dict(queued=1)),
    "F": ({T.RMD_TUNE_PATH_QUEUES: 1, T.RMD_TUNE_CHAIN_ITEMS: 2, T.RMD_TUNE_LAUNCH_FORM: 2}, {}, dict(chained=1, queued=0, buffered=1)),
    "G": ({T.RMD_TUNE_SAMPLE_SPLIT: 3, T.RMD_TUNE_LAUNCH_FORM: 1}, {}, dict(persistent=0, buffered=1)),
    "H": ({}, {}, {}),
    "I-general-planes": (B, {T.RMD_TUNE_AXIS_PAIRS: 1}, dict(queued=1)),
    "I-coarse-masks": (B, {T.RMD_TUNE_MASK_BUDGET: 256}, dict(queued=1)),
    "K-B-batch-1": ({**B, T.RMD_TUNE_WALK_BATCH: 1}, {}, dict(queued=1)),
    "K-B-batch-1000": ({**B, T.RMD_TUNE_WALK_BATCH: 1000}, {}, dict(queued=1)),
    "K-A-batch-1": ({**A, T.RMD_TUNE_WALK_BATCH: 1}, {}, dict(buffered=0, queued=0)),
    "K-A-batch-1000": ({**A, T.RMD_TUNE_WALK_BATCH: 1000}, {}, dict(buffered=0, queued=0)),
}


@pytest.fixture(scope="module")
def ctx(product_lib):
    """A context of this module's own: the tests change its tunables."""
    with render.Context(0) as c:
        yield c


def equal_frames(name, a, b):
    if name in ms.NAN_FOR_NAN:
        from test_gpu_parity import same_bits

        return a.shape == b.shape and bool(same_bits(a, b).all())
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def prefill(case, W, H, salt=0):
    return np.random.default_rng([salt, case[1], int(case[2]), len(case[0])]).uniform(0.25, 3.0, (H, W, 3))


def info_dict(info):
    return {k: int(getattr(info, k)) for k in INFO_FIELDS}


class Forms:
    """One case's scene on the device and the ways to render its samples."""

    def __init__(self, ctx, case, mode=0):
        self.ctx, self.case = ctx, case
        flags = ms.render_flags(case)[mode - 1] if mode else {}
        self.scene, self.cam, self.st, self.note = ms.build(case, **flags)
        self.W, self.H, self.spp = self.cam.backbuffer_width, self.cam.backbuffer_height, self.st.sample_count
        self.tiles = generate_tiles(self.W, self.H, self.st.tile_size)
        self.open, self.scenes = [], {}

    def set(self, tunables):
        for key in KEYS:
            self.ctx.set_tunable(key, tunables.get(key, 0))

    def device_scene(self, under=None):
        """the scene as created under the case's own tunables and `under` (read when the scene is created); one upload per setting"""
        under = {**ms.scene_tunables(self.case), **(under or {})}
        key = tuple(sorted(under.items()))
        if key not in self.scenes:
            self.set(under)
            try:
                self.scenes[key] = render.DeviceScene(self.ctx, self.scene)
            finally:
                self.set({})
            self.open.append(self.scenes[key])
        return self.scenes[key]

    def framebuffer(self):
        fb = render.Framebuffer(self.ctx, self.W, self.H)
        self.open.append(fb)
        return fb

    def close(self):
        self.set({})
        for o in self.open:
            o.close()

    def render(self, ds, fb, base, tunables, ranges=None, tiles=None, fb_sq=None, base_sq=None):
        """-> (frame, squares or None, launch info of the last launch as a dict)"""
        self.set(tunables)
        try:
            fb.zero() if base is None else fb.upload(base)
            if fb_sq is not None:
                fb_sq.upload(base_sq)
            for begin, count in ranges or [(0, self.spp)]:
                render.render_tiles(self.ctx, ds, self.cam, self.st, self.tiles if tiles is None else tiles, fb, begin, count, framebuffer_sq=fb_sq)
            return fb.download(), (fb_sq.download() if fb_sq is not None else None), info_dict(self.ctx.last_launch_info())
        finally:
            self.set({})


def check_scene_plan(f, ds):
    """what rmd_scene_create decided, against what the class names"""
    from test_mesh_scenes_host import without_grids

    name, seed, _ = f.case
    plan = probe.scene_plan(ds)
    at, grids = ms.grid_objects(f.scene), ms.distinct_grids(f.scene)
    launch_visit, launch_pairs, _, _, _ = probe.primary_candidates(f.cam, f.st, f.scene, [(0, 0, 8, 8)])
    print("%s: scene plan %s" % (ms.case_id(f.case), plan))
    assert plan["n_grid_objects"] == len(at) and plan["n_grids"] == len(grids) == len(plan["mask_shift"])
    assert plan["grid_mask"] == sum(1 << i for i in at if i < 64) and plan["visit_mask"] == launch_visit and plan["axis_pairs"] == launch_pairs
    assert plan["walk_steps_bound"] == max(sum(int(v) for v in g.resolution) + 3 for g in grids)
    assert probe.scene_layout(ds)[:2] == (len(f.scene.objects), len(grids))
    if name == "shared_grid":
        assert plan["n_grid_objects"] == 2 and plan["n_grids"] == (1 if seed < 2 else 2)
    if name == "three_grids":
        assert plan["n_grid_objects"] == 3 and (all(s > 0 for s in plan["mask_shift"]) if seed >= 2 else plan["mask_shift"] == [0, 0, 0]), plan
    if name == "one_cell":
        assert plan["walk_steps_bound"] == (6, 7, 8)[seed]
    if name == "open_scene":
        assert plan["axis_pairs"] == 0
    if name == "materials":
        assert plan["regular"] == int(ss.is_regular(without_grids(f.scene)))
    if name not in ("shared_grid", "three_grids") and len(at) == 1:
        assert plan["n_grid_objects"] == 1  # (the only scenes whose walks may be put aside)
    return plan


@pytest.mark.parametrize("case,mode", MODES, ids=MODE_IDS)
def test_every_launch_form_gives_form_a_byte_for_byte(ctx, case, mode):
    name = case[0]
    f = Forms(ctx, case, mode)
    try:
        base, base_sq = prefill(case, f.W, f.H), prefill(case, f.W, f.H, salt=1)
        ds, fb, fb_sq = f.device_scene(), f.framebuffer(), f.framebuffer()
        check_scene_plan(f, ds)
        a, _, info = f.render(ds, fb, base, A)
        assert info["buffered"] == 0 and info["queued"] == 0 and info["has_grid"] == 1, info
        assert (a != base).any(), "%s: form A left the pre-fill as it was" % ms.case_id(case)  # (no case is black by construction)
        frames, infos = {}, {}
        for key, (tunables, under, want) in FORMS.items():
            frames[key], _, infos[key] = f.render(f.device_scene(under), fb, base, tunables)
            assert all(infos[key][k] == v for k, v in want.items()), "%s form %s: launched as %s, wanted %s" % (ms.case_id(case), key, infos[key], want)
        assert infos["D"]["passes"] >= 2, infos["D"]
        coarse = probe.scene_plan(f.device_scene({T.RMD_TUNE_MASK_BUDGET: 256}))
        print("%s form H: %s; mask shifts under a budget of 256 bytes: %s" % (ms.case_id(case), infos["H"], coarse["mask_shift"]))
        if name == "grid_positions":  # the object table is inside the LDS plan of the persistent form
            assert infos["B"]["persistent"] == 1 and infos["F"]["persistent"] == 1
        frames["J"], _, info = f.render(ds, fb, base, B, ranges=[(0, FIRST_LAUNCH), (FIRST_LAUNCH, f.spp - FIRST_LAUNCH)])
        assert info["queued"] == 1
        a_sum, a_sq, info = f.render(ds, fb, base, A, fb_sq=fb_sq, base_sq=base_sq)
        assert info["buffered"] == 0 and info["queued"] == 0
        frames["L"], l_sq, info = f.render(ds, fb, base, B, fb_sq=fb_sq, base_sq=base_sq)
        assert info == infos["B"], "the moments launch took another form: %s vs %s" % (info, infos["B"])
        for key, img in frames.items():
            diff = ~((img == a) | (np.isnan(img) & np.isnan(a)))
            print("%s form %s: %d of %d values differ from form A%s" % (ms.case_id(case), key, diff.sum(), a.size, "" if not diff.any() else
                  ", first at (y, x, c) %s: %r vs %r" % (tuple(np.argwhere(diff)[0]), img[tuple(np.argwhere(diff)[0])], a[tuple(np.argwhere(diff)[0])])))
        for key, img in frames.items():
            assert equal_frames(name, img, a), "%s: form %s differs from form A (%s)" % (ms.case_id(case), key, f.note)
        assert equal_frames(name, a_sum, a) and equal_frames(name, l_sq, a_sq), "%s: the moments differ between forms A and B" % ms.case_id(case)
        assert (a_sq != base_sq).any()
    finally:
        f.close()


@pytest.mark.parametrize("case", RECT_CASES, ids=[ms.case_id(c) for c in RECT_CASES])
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
            a, _, info = f.render(ds, fb, base, A, tiles=rects)
            assert info["buffered"] == 0 and info["queued"] == 0
            b, _, info = f.render(ds, fb, base, B, tiles=rects)
            assert info["queued"] == 1 and info["buffered"] == 1
            assert a.tobytes() == b.tobytes(), "%s: forms A and B differ over %s" % (ms.case_id(case), rects[:2])
            assert a[~covered].tobytes() == base[~covered].tobytes(), "%s: a pixel no rect covers lost its pre-fill" % ms.case_id(case)
            assert (a[covered] != base[covered]).any()
    finally:
        f.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_queued_form_agrees_with_the_oracle(ctx, oracle, case):
    from test_gpu_fullsize import account_for_off_pixels, rel_close  # the suite's per-pixel bar

    f = Forms(ctx, case)
    try:
        dev, _, info = f.render(f.device_scene(), f.framebuffer(), None, B)
        assert info["queued"] == 1 and info["has_grid"] == 1
    finally:
        f.close()
    ref = oracle.OracleScene(f.scene).render_tiles(f.cam, f.st, f.tiles, threads=16)
    ok = rel_close(dev, ref, 1e-9).all(axis=2)
    account_for_off_pixels(ctx, oracle, f.scene, f.st, f.cam, f.spp, dev, ref, ok, "mesh scenes %s" % ms.case_id(case))


@pytest.mark.parametrize("case", ms.cases(("materials",)), ids=[ms.case_id(c) for c in ms.cases(("materials",))])
def test_black_path_modes_change_no_finite_sample(ctx, case):
    """flags 0 traces black paths on in a scene with a grid: identical to TRACE; END may differ only where the flags-0 frame is non-finite"""
    from test_gpu_parity import same_bits

    frames = {}
    for mode, label in enumerate(("default", "trace", "end")):
        assert [(), ("trace_black_paths",), ("end_black_paths",)][mode] == tuple(ms.render_flags(case)[mode - 1] if mode else ())
        f = Forms(ctx, case, mode)
        try:
            frames[label], _, info = f.render(f.device_scene(), f.framebuffer(), None, B)
            assert info["queued"] == 1 and info["end_black_paths"] == (1 if label == "end" else 0), (label, info)
        finally:
            f.close()
    assert same_bits(frames["default"], frames["trace"]).all()
    same = same_bits(frames["end"], frames["default"]).all(axis=2)
    assert np.isfinite(frames["default"][~same]).all(axis=1).sum() == 0, "%s: a finite pixel changed" % ms.case_id(case)
    print("%s: %d pixels differ under END_BLACK_PATHS, all non-finite in the flags-0 frame" % (ms.case_id(case), (~same).sum()))


DIAG_CHILD = r"""
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import mesh_scenes as ms
from raymond_amd import abi, lib, render
from raymond_amd.scene import generate_tiles

assert lib.LIB_PATH.endswith("diag/libraymond_hip.so"), lib.LIB_PATH
os.environ["RMD_DEBUG"] = "72"  # 8: event counters, 64: every pair the sphere pre-test drops ALSO takes the reference's triangle test
for case in ms.cases(%(classes)r, lens=False):
    scene, cam, st, note = ms.build(case)
    W, H = cam.backbuffer_width, cam.backbuffer_height
    with render.Context(0) as ctx:
        for key, value in ms.scene_tunables(case).items():
            ctx.set_tunable(key, value)
        ds, fb = render.DeviceScene(ctx, scene), render.Framebuffer(ctx, W, H)
        for key in ms.scene_tunables(case):
            ctx.set_tunable(key, 0)
        ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 2)  # form B
        sys.stderr.write("== %%s\n" %% ms.case_id(case)), sys.stderr.flush()
        render.render_tiles(ctx, ds, cam, st, generate_tiles(W, H, st.tile_size), fb)
        info = ctx.last_launch_info()
        assert info.queued == 1 and info.persistent == 1 and info.has_grid == 1 and info.passes == 1, case
        fb.close(), ds.close()
print("mesh scenes ok")
"""


def test_the_queued_form_counts_what_the_classes_name_in_the_diag_build(product_lib):
    assert os.path.exists(DIAG_LIB), "build the DIAG library: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, RAYMOND_HIP_LIB=DIAG_LIB)
    env.pop("RMD_DEBUG", None)
    r = subprocess.run([sys.executable, "-c", DIAG_CHILD % {"root": ROOT, "classes": DIAG_CLASSES}], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "mesh scenes ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    seen, name = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("== "):
            name = line[3:]
            seen[name] = dict(passed=0, dropped_wrongly=0, pushed=0, aside=0, held=0, lines=0)
        m = re.search(r"sphere pre-test: pairs passed=(\d+) full chunks=\d+ .*\(flag 64; must be 0\)=(\d+)", line)
        if m and name:
            seen[name]["passed"] += int(m.group(1))
            seen[name]["dropped_wrongly"] += int(m.group(2))
            seen[name]["lines"] += 1
        m = re.search(r"path queues: rays pushed=(\d+) \(of them walks put aside=(\d+)\) rays held in their lanes=(\d+)", line)
        if m and name:
            for k, v in zip(("pushed", "aside", "held"), m.groups()):
                seen[name][k] += int(v)
            seen[name]["lines"] += 1
    print(seen)
    cases = ms.cases(DIAG_CLASSES, lens=False)
    assert sorted(seen) == sorted(ms.case_id(c) for c in cases), r.stderr[-3000:]
    by_class = {c: dict(passed=0, aside=0, held=0, pushed=0) for c in DIAG_CLASSES}
    for case in cases:
        d = seen[ms.case_id(case)]
        assert d["lines"] == 2, (case, d)  # one launch, both lines
        assert d["dropped_wrongly"] == 0, (case, d)
        for k in by_class[case[0]]:
            by_class[case[0]][k] += d[k]
        if case[0] in ("shared_grid", "three_grids"):  # two or three grid objects: the carried state is one walk's, so no walk is put aside
            assert d["aside"] == 0 and d["passed"] > 0 and d["pushed"] + d["held"] > 0, (case, d)
        if case[0] == "no_ray_enters" and case[1] < 2:  # the open variant: no ray of the frame enters the box
            assert d["pushed"] == 0 and d["held"] == 0 and d["passed"] == 0 and d["aside"] == 0, (case, d)
    for c in ("shared_grid", "three_grids", "every_ray_walks", "mirror_box"):  # the classes that have walks
        assert by_class[c]["passed"] > 0, (c, by_class[c])
    assert by_class["every_ray_walks"]["held"] > 0 and by_class["every_ray_walks"]["pushed"] > 0, by_class["every_ray_walks"]
    assert max(by_class[c]["aside"] for c in ("every_ray_walks", "mirror_box", "no_ray_enters")) > 0, by_class  # walks ARE put aside with one grid object
