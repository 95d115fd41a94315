"""The feature-slope term of the guided non-local-means filters (rmd_denoise_guided_slope, rmd_denoise_dual_guided_slope, its region form and
rmd_denoise_dual_select_slope): the parts that need no GPU.

The four entry points are exported and declared as the header states them; every argument rule of the call without the suffix holds for them, in the same
order and with the same text but for the name (the recorded cases of tests/golden/denoise_refusals.json are replayed against them), and the slope has its
own rule; Settings.check_denoise and the C++ mirror refuse what they should; the numpy restatement (tests/denoise_slope_ref.py) keeps the definition's
consequences; and the scratch block holds the slope planes only when a slope is > 0, behind the feature planes.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_dual_guided_ref as dgref
import denoise_dual_select_ref as sref
import denoise_guided_ref as gref
import denoise_slope_ref as slref
from raymond_amd import abi, lib, probe, scenes
from raymond_amd.scene import Settings
from test_denoise_dual_select_host import _frame
from test_denoise_refusals_host import rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
# the new call -> the call without the suffix, the argument the new one follows, and its number of arguments
NEW = {
    "rmd_denoise_guided_slope": ("rmd_denoise_guided", "tau", 18),
    "rmd_denoise_dual_guided_slope": ("rmd_denoise_dual_guided", "tau", 23),
    "rmd_denoise_dual_guided_slope_region": ("rmd_denoise_dual_guided_region", "tau", 25),
    "rmd_denoise_dual_select_slope": ("rmd_denoise_dual_select", "cands", 25),
}
with open(os.path.join(ROOT, "tests", "golden", "denoise_refusals.json")) as _f:
    GOLDEN = json.load(_f)


# ---------------------------------------------------------------- the boundary
def test_the_four_entry_points_are_exported_declared_and_mirrored(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    fault_list = header[header.index("RMD_ERR_DEVICE_FAULT = 8") : header.index("};", header.index("RMD_ERR_DEVICE_FAULT = 8"))]
    rs, doc = open(os.path.join(ROOT, "integration", "gpu.rs")).read(), open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, (base, after, n_args) in NEW.items():
        assert name in exported and base in exported
        assert len(lib.SIGNATURES[name][1]) == n_args == len(lib.SIGNATURES[base][1]) + 1
        # the declaration is the base call's with one argument more, right behind `after`
        decl = re.search(r"rmd_status %s\((.*?)\);" % name, header).group(1)
        base_decl = re.search(r"rmd_status %s\((.*?)\);" % base, header).group(1)
        if after == "tau":
            assert decl == base_decl.replace("double tau, ", "double tau, double slope, ")
        else:
            assert decl == base_decl.replace("const rmd_denoise_candidate *cands, ", "const rmd_denoise_candidate *cands, const double *cand_slopes, ")
        assert name in fault_list and "fn %s(" % name in rs and "pub fn %s(" % name in doc
    assert "#define RMD_ABI_VERSION 6u" in header  # additions within ABI 6
    # the ctypes mirrors: the base call's list with the slope (a double; select: a pointer to doubles) where the header has it
    g, b = lib.SIGNATURES["rmd_denoise_guided_slope"][1], lib.SIGNATURES["rmd_denoise_guided"][1]
    assert g == b[:-1] + [C.c_double] + b[-1:]
    for name in ("rmd_denoise_dual_guided_slope", "rmd_denoise_dual_guided_slope_region"):
        g, b = lib.SIGNATURES[name][1], lib.SIGNATURES[NEW[name][0]][1]
        assert g == b[:-2] + [C.c_double] + b[-2:]
    g, b = lib.SIGNATURES["rmd_denoise_dual_select_slope"][1], lib.SIGNATURES["rmd_denoise_dual_select"][1]
    assert g == b[:17] + [C.POINTER(C.c_double)] + b[17:]


def _call(L, name, kw, slope):
    """rec.call for a _slope entry point: the base call's arguments from `kw`, `slope` (select: the cand_slopes tuple or None) behind NEW[name]'s argument."""
    base, after, _ = NEW[name]
    keep, args = [], []
    for key, good in rec.ENTRY_POINTS[base]:
        v = kw.get(key, good)
        if key in ("rects", "region"):
            v = rec._rects(v)
        elif key == "cands" and v is not None:
            v = (abi.DenoiseCandidate * len(v))(*(abi.DenoiseCandidate(**c) for c in v))
        elif v == "counts":
            v = (C.c_uint32 * 4)(4, 4, 4, 4)
        args.append(v)
        if key == after:
            args.append(slope if after == "tau" else None if slope is None else (C.c_double * len(slope))(*slope))
        keep.append(args[-1])
    status = getattr(L, name)(None, *args)
    del keep
    return int(status), (L.rmd_last_error(None) or b"").decode()


@pytest.mark.parametrize("name", list(NEW))
def test_every_recorded_case_of_the_call_without_the_suffix_is_answered_alike(product_lib, name):
    """The same status and the same text with the new call's name in front, for every single fault, every ordered pair and every valid variant, at a
    good slope: the new calls share the checks of the old ones and their order."""
    base = NEW[name][0]
    e = GOLDEN["entry_points"][base]
    n = len(e["singles"])
    pair = ((i, j) for i in range(n) for j in range(n) if i != j)
    slope = 3.0 if NEW[name][1] == "tau" else (0.0, 3.0, 0.0, 3.0, 0.0)
    replayed = 0
    for kind, cid, kw in rec.cases(base):
        if kind == "pairs":
            i, j = next(pair)
            status, text = e["outcomes"][rec.CELLS.index(e["pairs"][i][j])]
        else:
            status, text = e["outcomes"][e[kind][cid]]
        if text.startswith(base + ": "):
            text = name + text[len(base) :]
        assert list(_call(product_lib, name, kw, slope)) == [status, text], (name, cid)
        replayed += 1
    assert replayed == n * n + len(e["valid"])


BAD_SLOPES = (-1e-300, -1.0, float("nan"), float("inf"), -float("inf"))


@pytest.mark.parametrize("name", [n for n in NEW if NEW[n][1] == "tau"])
def test_the_slope_rule_without_a_device(product_lib, name):
    L = product_lib
    want = name + ": slope must be finite and >= 0"
    for bad in BAD_SLOPES:
        assert _call(L, name, {}, bad) == (abi.RMD_ERR_INVALID_ARGUMENT, want), bad
        # it is checked after k_f and tau, and before the rects
        assert "tau must" in _call(L, name, dict(tau=0.0), bad)[1] and "k_f must" in _call(L, name, dict(kf=-1.0), bad)[1]
        assert _call(L, name, dict(rects=((0, 0, 9, 8),)), bad)[1] == want
        # without features it is not read
        off = dict(F=None, G=None, cf=None) if "dual" in name else dict(F=None, G=None)
        assert _call(L, name, off, bad) == (abi.RMD_ERR_INVALID_ARGUMENT, "null context")
    for good in (0.0, -0.0, 1e-300, 3.0, 1e300):
        assert _call(L, name, {}, good) == (abi.RMD_ERR_INVALID_ARGUMENT, "null context"), good


def test_the_candidate_slopes_rule_without_a_device(product_lib):
    L, name = product_lib, "rmd_denoise_dual_select_slope"
    for bad in BAD_SLOPES:
        assert _call(L, name, {}, (0.0, bad)) == (abi.RMD_ERR_INVALID_ARGUMENT, name + ": candidate 1: slope must be finite and >= 0"), bad
        assert _call(L, name, {}, (bad, 3.0)) == (abi.RMD_ERR_INVALID_ARGUMENT, "null context")  # candidate 0 is not guided: its slope is not read
        assert "candidate 1: tau must" in _call(L, name, dict(cands=(rec.CAND, dict(rec.GUIDED, tau=0.0))), (0.0, bad))[1]
        assert "slope must" in _call(L, name, dict(rects=((0, 0, 9, 8),)), (0.0, bad))[1]
        assert _call(L, name, dict(F=None, G=None, cf=None, cands=(rec.CAND, rec.CAND)), (bad, bad)) == (abi.RMD_ERR_INVALID_ARGUMENT, "null context")
    for good in (None, (0.0, 0.0), (0.0, 3.0), (7.0, 1e300)):
        assert _call(L, name, {}, good) == (abi.RMD_ERR_INVALID_ARGUMENT, "null context"), good


# ---------------------------------------------------------------- the settings and their C++ mirror
def test_settings_feature_slope_rules():
    cam = scenes.camera(64, 64)
    assert Settings(cam, 16).denoise_feature_slope == 0.0 and Settings(cam, 16).slope_keyword() == {}
    single = dict(denoise=True, denoise_features=True)
    dual = dict(denoise=True, denoise_dual=True, samples_per_iteration=8)
    st = Settings(cam, 16, denoise_feature_slope=3, **single)
    assert st.denoise_feature_slope == 3.0 and st.slope_keyword() == dict(slope=3.0)
    Settings(cam, 64, denoise_dual_features=True, denoise_feature_slope=0.5, adaptive_denoised_threshold=0.01, **dual)
    st = Settings(cam, 64, denoise_dual_select=True, denoise_feature_slope=2.0, **dual)
    assert st.select_candidates() == [dict(k=0.45, alpha=1.0), dict(k=1.0, alpha=1.0, guided=True, k_f=1.0, tau=1e-2, slope=2.0)]
    assert "slope" not in Settings(cam, 64, denoise_dual_select=True, **dual).select_candidates()[1]  # off: the candidates of before
    for bad in BAD_SLOPES[1:]:
        with pytest.raises(ValueError, match="denoise_feature_slope must be finite and >= 0"):
            Settings(cam, 16, denoise_feature_slope=bad, **single)
        with pytest.raises(ValueError, match="denoise_feature_slope must be finite and >= 0"):
            Settings(cam, 16, denoise_feature_slope=bad)  # checked whether or not a filter is on
    for off in (dict(), dict(denoise=True), dual):
        with pytest.raises(ValueError, match="needs a guided non-local-means filter"):
            Settings(cam, 64, denoise_feature_slope=3.0, **off)
        Settings(cam, 64, denoise_feature_slope=0.0, **off)
    with pytest.raises(ValueError, match="cannot be combined with denoise_atrous / denoise_dual_atrous"):
        Settings(cam, 16, denoise_atrous=True, denoise_feature_slope=3.0, **single)
    with pytest.raises(ValueError, match="cannot be combined with denoise_atrous / denoise_dual_atrous"):
        Settings(cam, 64, denoise_dual_features=True, denoise_dual_atrous=True, denoise_feature_slope=3.0, **dual)
    st = Settings(cam, 16, denoise_feature_slope=3.0, **single)
    st.denoise_feature_slope = float("nan")
    from raymond_amd import render

    with pytest.raises(ValueError, match="denoise_feature_slope"):
        render.render_tiled(scenes.reflective_spheres(), st)  # refused again before a context is created


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


def test_cli_feature_slope_rules(cli, tmp_path):
    """render_tiled (C++) throws raymond::Error before it starts a worker: no device is needed to see it."""
    head = [cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm")]

    def refused(*opts):
        r = subprocess.run(head + list(opts), capture_output=True, text=True)
        assert r.returncode == 1, (opts, r.stderr)
        return r.stderr

    single, dual = ["--denoise", "1", "--denoise-features", "1"], ["--denoise", "1", "--spi", "4", "--denoise-dual", "1"]
    for bad in ("-1", "nan", "inf"):
        assert "denoise_feature_slope must be finite and >= 0" in refused(*single, "--denoise-feature-slope", bad)
    for off in ([], ["--denoise", "1"], dual):
        assert "denoise_feature_slope > 0 needs a guided non-local-means filter" in refused(*off, "--denoise-feature-slope", "3")
    assert "denoise_feature_slope cannot be combined with denoise_atrous / denoise_dual_atrous" in refused(*single, "--denoise-atrous", "1", "--denoise-feature-slope", "3")
    assert "denoise_feature_slope cannot be combined with denoise_atrous / denoise_dual_atrous" in refused(*dual, "--denoise-dual-features", "1", "--denoise-dual-atrous", "1",
                                                                                                        "--denoise-feature-slope", "3")
    usage = open(os.path.join(ROOT, "raymond_amd", "host", "cli.cpp")).read().split("#include")[0]  # the usage text is that file's header
    assert "[--denoise-feature-slope G]" in usage
    undefined = subprocess.run(["nm", "-D", "--undefined-only", cli], check=True, capture_output=True, text=True).stdout
    for name in NEW:
        assert name + "\n" in undefined


# ---------------------------------------------------------------- the restatement's own properties
def _single_frame(W, H):
    halves, F, G, n_f = _frame(W, H)
    return halves[0], halves[1], F, G, halves[4]


def test_slope_zero_is_the_existing_restatements_bit_for_bit():
    W, H = 13, 9
    S, Q, F, G, n = _single_frame(W, H)
    for kw in (dict(k_f=1.0, tau=1e-2), dict(k_f=0.6, tau=1e-3)):
        a = slref.denoise_guided_slope(S, Q, F, G, n, radius=3, patch_radius=1, slope=0.0, **kw)
        assert a.tobytes() == gref.denoise_guided(S, Q, F, G, n, radius=3, patch_radius=1, **kw).tobytes()
        assert np.isnan(a).any() and np.isfinite(a).any()
    for frame in (gref.step_edge_frame(1), slref.dome_frame(1)[:6]):
        S, Q, F, G, n, _ = frame
        assert slref.denoise_guided_slope(S, Q, F, G, n, slope=0.0).tobytes() == gref.denoise_guided(S, Q, F, G, n, k_f=1.0, tau=1e-2).tobytes()
    halves, F, G, n_f = _frame(W, H)
    out, err = slref.denoise_dual_guided_slope(*halves, F, G, n_f, radius=3, patch_radius=1, slope=0.0)
    want = dgref.denoise_dual_guided(*halves, F, G, n_f, radius=3, patch_radius=1)
    assert out.tobytes() == want[0].tobytes() and err.tobytes() == want[1].tobytes()
    cands = [dict(k=0.45), dict(k=1.0, guided=True, k_f=1.0, tau=1e-2)]
    zero = [dict(c, slope=0.0) for c in cands]
    a = slref.denoise_dual_select_slope(*halves, zero, F, G, n_f, radius=3, patch_radius=1)
    b = sref.denoise_dual_select(*halves, cands, F, G, n_f, radius=3, patch_radius=1)
    assert all(a[name].tobytes() == b[name].tobytes() for name in ("out", "err", "sure", "win"))


def test_slope_planes_are_the_definition_read_pixel_by_pixel():
    """The vectorised planes against Python loops over the header's lines, on features with misses, poison and every kind of border."""
    for W, H in ((1, 1), (2, 1), (1, 3), (3, 3), (13, 9)):
        S, Q, F, G, n = _single_frame(W, H)
        _, _, valid = slref.mean_and_variance(S, Q, n)
        ff, gg, fvalid = gref.feature_mean_and_variance(F, G, n, valid)
        m = slref.slope_planes(ff, fvalid, 1.5)
        s2 = 1.5 * 1.5
        for y in range(H):
            for x in range(W):
                for j in range(7):
                    want = 0.0
                    if fvalid[y, x]:
                        axes = []
                        for (ay, ax), (by, bx) in (((y, x - 1), (y, x + 1)), ((y - 1, x), (y + 1, x))):
                            both = 0 <= ay and 0 <= ax and by < H and bx < W and fvalid[ay, ax] and fvalid[by, bx]
                            a_l, a_r = (ff[y, x, j] - ff[ay, ax, j], ff[by, bx, j] - ff[y, x, j]) if both else (0.0, 0.0)
                            axes.append((a_l * a_l if a_l * a_l < a_r * a_r else a_r * a_r) if both else 0.0)
                        want = s2 * (axes[0] + axes[1])
                    assert m[y, x, j] == want, (W, H, x, y, j)
        if W * H > 9:
            assert (m > 0).any() and (~fvalid).any() and (m[~fvalid] == 0).all()


@pytest.mark.parametrize("frame", ["step1", "step2", "hit_miss"])
def test_features_with_a_flat_side_give_the_slope_zero_bytes(frame):
    """A step has a flat side at every pixel, so no slope counts: an edge stays an edge, and a miss never mixes with a hit."""
    S, Q, F, G, n, _ = gref.hit_miss_frame() if frame == "hit_miss" else gref.step_edge_frame(int(frame[-1]))
    zero = slref.denoise_guided_slope(S, Q, F, G, n, slope=0.0)
    for slope in (1.0, 3.0, 8.0):
        assert slref.denoise_guided_slope(S, Q, F, G, n, slope=slope).tobytes() == zero.tobytes(), slope
    if frame == "hit_miss":
        assert zero.tobytes() == gref.hit_miss_frame()[5].tobytes()


def test_a_miss_alone_between_hits_has_a_two_sided_slope_and_mixes():
    """The header's caveat: "a miss never mixes with a hit" holds for a miss that has another miss beside it.  One miss pixel with hits on both sides
    on both axes has a depth slope of the whole depth on each, so at any slope > 0 ITS value takes the hits around it; the hits, flat on their
    other side, still leave it out."""
    S, Q, F, G, n, u = gref.hit_miss_frame()
    y, x = 12, 10  # inside the hits (columns 0 .. 24), further than the radius from the misses
    S, Q, F, G, u = S.copy(), Q.copy(), F.copy(), G.copy(), u.copy()
    u[y, x] = 0.75
    S[y, x] = u[y, x] * n[y, x]
    Q[y, x] = S[y, x] * u[y, x] + 0.5 * n[y, x] * (n[y, x] - 1)
    F[y, x], G[y, x] = 0.0, 0.0
    zero = slref.denoise_guided_slope(S, Q, F, G, n, slope=0.0)
    assert zero.tobytes() == u.tobytes()  # slope 0: it keeps to itself, exactly
    for slope in (0.5, 3.0):
        got = slref.denoise_guided_slope(S, Q, F, G, n, slope=slope)
        assert np.all(np.abs(got[y, x] - 0.75) > 0.3), slope  # the miss is now mostly its neighbours' 0.25
        rest = np.ones(n.shape, dtype=bool)
        rest[y, x] = False
        assert got[rest].tobytes() == u[rest].tobytes(), slope  # every other pixel is untouched: the hits do not take the miss


@pytest.mark.parametrize("seed", [1, 2])
def test_the_dome_is_filtered_as_a_surface(seed):
    """On a curved surface of one colour the guided filter reads every normal as an edge; at slope 3 the disc's RMSE is at most 0.6 of slope 0's (the
    issue's bar; measured 0.412 on seed 1 and 0.430 on seed 2)."""
    S, Q, F, G, n, truth, disc = slref.dome_frame(seed)
    kw = dict(radius=10, patch_radius=3, k=0.45, alpha=1.0, k_f=1.0, tau=1e-2)
    r0 = slref.disc_rmse(slref.denoise_guided_slope(S, Q, F, G, n, slope=0.0, **kw), truth, disc)
    r3 = slref.disc_rmse(slref.denoise_guided_slope(S, Q, F, G, n, slope=3.0, **kw), truth, disc)
    print("dome seed %d: disc RMSE slope 0 %.5f slope 3 %.5f ratio %.3f" % (seed, r0, r3, r3 / r0))
    assert r3 <= 0.6 * r0


# ---------------------------------------------------------------- the scratch block
@pytest.mark.parametrize("form", ["single", "dual", "dual_select"])
def test_the_slope_planes_exist_only_with_a_slope_and_lie_behind_the_feature_planes(form):
    for (W, H), n_rects, n_table in (((1, 1), 0, 0), ((37, 23), 3, 0), ((45, 29), 1, 5)):
        n_cands = 2 if form == "dual_select" else 0
        N = W * H
        before = probe.denoise_scratch(form, W, H, n_rects, True, n_cands, n_table)
        off = probe.denoise_scratch(form, W, H, n_rects, True, n_cands, n_table, sloped=False)
        on = probe.denoise_scratch(form, W, H, n_rects, True, n_cands, n_table, sloped=True)
        assert off == before and "slope_planes" not in off[0]  # slope 0: the block of the call without the suffix
        parts, total = on
        assert parts["slope_planes"] == (parts["feat_planes"][0] + (8 * 14 * N + 15) // 16 * 16, 8 * 7 * N)
        assert set(parts) == set(before[0]) | {"slope_planes"} and all(parts[k][1] == before[0][k][1] for k in before[0])
        spans = sorted((o, o + b) for o, b in parts.values())
        assert all(o % 16 == 0 for o, _ in spans) and all(a_end <= b_begin for (_, a_end), (b_begin, _) in zip(spans, spans[1:]))
        assert total == sum((b + 15) // 16 * 16 for _, b in parts.values()) == before[1] + (8 * 7 * N + 15) // 16 * 16
        # parts in front of the feature planes stay where they were
        assert all(parts[k][0] == before[0][k][0] for k in before[0] if before[0][k][0] <= before[0]["feat_planes"][0])
        # without features there is nothing to take a slope of
        assert probe.denoise_scratch(form, W, H, n_rects, False, n_cands, n_table, sloped=True) == probe.denoise_scratch(form, W, H, n_rects, False, n_cands, n_table)


@pytest.mark.parametrize("form", [f for f in probe.SCRATCH_FORMS if f not in ("single", "dual", "dual_select")])
def test_the_other_forms_have_no_slope_planes(form):
    guided = form != "tile_error"
    assert probe.denoise_scratch(form, 37, 23, 3, guided, 0, 5, sloped=True) == probe.denoise_scratch(form, 37, 23, 3, guided, 0, 5)
