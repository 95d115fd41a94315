"""The feature-slope term of the guided a-trous filters (rmd_denoise_atrous_slope, rmd_denoise_atrous_dual_slope and its region form): the parts that
need no GPU.

The three entry points are exported, declared as the call without the suffix with `double slope` after `double tau`, and mirrored in ctypes; they refuse
what the calls without the suffix refuse, in the same order and with the same text but for the name (the recorded cases of
tests/golden/denoise_refusals.json are replayed against them), and the slope has its own rule; Settings.check_denoise and the C++ mirror know
denoise_atrous_slope; the numpy restatement (tests/denoise_atrous_slope_ref.py) keeps the definition's consequences in two readings; and the scratch
block holds the slope planes only when the slope is > 0, behind every other part.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_atrous_dual_ref as adref
import denoise_atrous_ref as aref
import denoise_atrous_slope_ref as asref
import denoise_guided_ref as gref
import denoise_slope_ref as slref
from raymond_amd import abi, lib, probe, scenes
from raymond_amd.scene import Settings
from test_denoise_dual_select_host import _frame
from test_denoise_refusals_host import rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
# the new call -> the call without the suffix and its number of arguments
NEW = {
    "rmd_denoise_atrous_slope": ("rmd_denoise_atrous", 17),
    "rmd_denoise_atrous_dual_slope": ("rmd_denoise_atrous_dual", 22),
    "rmd_denoise_atrous_dual_slope_region": ("rmd_denoise_atrous_dual_region", 24),
}
with open(os.path.join(ROOT, "tests", "golden", "denoise_refusals.json")) as _f:
    GOLDEN = json.load(_f)


# ---------------------------------------------------------------- the boundary
def test_the_three_entry_points_are_exported_declared_and_mirrored(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    fault_list = header[header.index("RMD_ERR_DEVICE_FAULT = 8") : header.index("};", header.index("RMD_ERR_DEVICE_FAULT = 8"))]
    for name, (base, n_args) in NEW.items():
        assert name in exported and base in exported
        assert len(lib.SIGNATURES[name][1]) == n_args == len(lib.SIGNATURES[base][1]) + 1
        decl = re.search(r"rmd_status %s\((.*?)\);" % name, header).group(1)
        base_decl = re.search(r"rmd_status %s\((.*?)\);" % base, header).group(1)
        assert decl == base_decl.replace("double tau, ", "double tau, double slope, ") != base_decl
        assert name in fault_list
    assert "#define RMD_ABI_VERSION 6u" in header  # additions within ABI 6
    assert "The a-trous filters have no slope form" not in header
    g, b = lib.SIGNATURES["rmd_denoise_atrous_slope"][1], lib.SIGNATURES["rmd_denoise_atrous"][1]
    assert g == b[:-1] + [C.c_double] + b[-1:]
    for name in ("rmd_denoise_atrous_dual_slope", "rmd_denoise_atrous_dual_slope_region"):
        g, b = lib.SIGNATURES[name][1], lib.SIGNATURES[NEW[name][0]][1]
        assert g == b[:-2] + [C.c_double] + b[-2:]


def _call(L, name, kw, slope):
    """rec.call for a _slope entry point: the base call's arguments from `kw`, `slope` behind tau."""
    keep, args = [], []
    for key, good in rec.ENTRY_POINTS[NEW[name][0]]:
        v = kw.get(key, good)
        if key in ("rects", "region"):
            v = rec._rects(v)
        elif v == "counts":
            v = (C.c_uint32 * 4)(4, 4, 4, 4)
        args.append(v)
        if key == "tau":
            args.append(slope)
        keep.append(args[-1])
    status = getattr(L, name)(None, *args)
    del keep
    return int(status), (L.rmd_last_error(None) or b"").decode()


@pytest.mark.parametrize("name", list(NEW))
def test_every_recorded_case_of_the_call_without_the_suffix_is_answered_alike(product_lib, name):
    """The same status and the same text with the new call's name in front, for every single fault, every ordered pair and every valid variant, at a
    good slope: the new calls go through the checks of the old ones, in their order."""
    base = NEW[name][0]
    e = GOLDEN["entry_points"][base]
    n = len(e["singles"])
    pair = ((i, j) for i in range(n) for j in range(n) if i != j)
    replayed = 0
    for kind, cid, kw in rec.cases(base):
        if kind == "pairs":
            i, j = next(pair)
            status, text = e["outcomes"][rec.CELLS.index(e["pairs"][i][j])]
        else:
            status, text = e["outcomes"][e[kind][cid]]
        if text.startswith(base + ": "):
            text = name + text[len(base) :]
        assert list(_call(product_lib, name, kw, 3.0)) == [status, text], (name, cid)
        replayed += 1
    assert replayed == n * n + len(e["valid"])


BAD_SLOPES = (-1e-300, -1.0, float("nan"), float("inf"), -float("inf"))


@pytest.mark.parametrize("name", list(NEW))
def test_the_slope_rule_without_a_device(product_lib, name):
    L = product_lib
    want = name + ": slope must be finite and >= 0"
    for bad in BAD_SLOPES:
        assert _call(L, name, {}, bad) == (abi.RMD_ERR_INVALID_ARGUMENT, want), bad
        # it is checked after k_f and tau, and before the rects (which are checked with the device bound)
        assert "tau must" in _call(L, name, dict(tau=0.0), bad)[1] and "k_f must" in _call(L, name, dict(kf=-1.0), bad)[1]
        assert _call(L, name, dict(rects=((0, 0, 9, 8),)), bad)[1] == want
        assert "levels must" in _call(L, name, dict(levels=9), bad)[1]  # ... and after the levels
        # without features it is not read: a NaN is accepted
        off = dict(F=None, G=None, cf=None) if "dual" in name else dict(F=None, G=None)
        assert _call(L, name, off, bad) == (abi.RMD_ERR_INVALID_ARGUMENT, "null context")
    for good in (0.0, -0.0, 1e-300, 3.0, 1e300):
        assert _call(L, name, {}, good) == (abi.RMD_ERR_INVALID_ARGUMENT, "null context"), good


# ---------------------------------------------------------------- the settings and their C++ mirror
SINGLE = dict(denoise=True, denoise_features=True, denoise_atrous=True)
DUAL = dict(denoise=True, denoise_dual=True, samples_per_iteration=8, denoise_dual_features=True, denoise_dual_atrous=True)
NEEDS = "denoise_atrous_slope > 0 needs a guided a-trous filter"


def test_settings_atrous_slope_rules():
    cam = scenes.camera(64, 64)
    assert Settings(cam, 16).denoise_atrous_slope == 0.0 and Settings(cam, 16).atrous_slope_keyword() == {}
    st = Settings(cam, 16, denoise_atrous_slope=3, **SINGLE)
    assert st.denoise_atrous_slope == 3.0 and st.atrous_slope_keyword() == dict(slope=3.0) and st.slope_keyword() == {}
    Settings(cam, 64, denoise_atrous_slope=0.5, adaptive_denoised_threshold=0.01, denoise_dual_atrous_region=True, **DUAL)
    assert Settings(cam, 16, **SINGLE).atrous_slope_keyword() == {}  # off: the calls of before
    for bad in BAD_SLOPES[1:]:
        with pytest.raises(ValueError, match="denoise_atrous_slope must be finite and >= 0"):
            Settings(cam, 16, denoise_atrous_slope=bad, **SINGLE)
        with pytest.raises(ValueError, match="denoise_atrous_slope must be finite and >= 0"):
            Settings(cam, 16, denoise_atrous_slope=bad)  # checked whether or not a filter is on
    offs = (dict(), dict(denoise=True), dict(denoise=True, denoise_atrous=True), dict(denoise=True, denoise_features=True),
            dict(DUAL, denoise_dual_features=False), dict(DUAL, denoise_dual_atrous=False))
    for off in offs:
        with pytest.raises(ValueError, match=NEEDS):
            Settings(cam, 64, denoise_atrous_slope=3.0, **off)
        Settings(cam, 64, denoise_atrous_slope=0.0, **off)
    # denoise_feature_slope keeps its own refusal of the a-trous filters, in its own words
    with pytest.raises(ValueError, match="denoise_feature_slope cannot be combined with denoise_atrous / denoise_dual_atrous"):
        Settings(cam, 16, denoise_feature_slope=3.0, denoise_atrous_slope=3.0, **SINGLE)
    st = Settings(cam, 16, denoise_atrous_slope=3.0, **SINGLE)
    st.denoise_atrous_slope = float("nan")
    from raymond_amd import render

    with pytest.raises(ValueError, match="denoise_atrous_slope"):
        render.render_tiled(scenes.reflective_spheres(), st)  # refused again before a context is created


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


def test_cli_atrous_slope_rules(cli, tmp_path):
    """render_tiled (C++) throws raymond::Error before it starts a worker: no device is needed to see it."""
    head = [cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm")]

    def refused(*opts):
        r = subprocess.run(head + list(opts), capture_output=True, text=True)
        assert r.returncode == 1, (opts, r.stderr)
        return r.stderr

    single = ["--denoise", "1", "--denoise-features", "1", "--denoise-atrous", "1"]
    dual = ["--denoise", "1", "--spi", "4", "--denoise-dual", "1", "--denoise-dual-atrous", "1"]
    for bad in ("-1", "nan", "inf"):
        assert "denoise_atrous_slope must be finite and >= 0" in refused(*single, "--denoise-atrous-slope", bad)
        assert "denoise_atrous_slope must be finite and >= 0" in refused("--denoise-atrous-slope", bad)
    for off in ([], ["--denoise", "1"], ["--denoise", "1", "--denoise-atrous", "1"], ["--denoise", "1", "--denoise-features", "1"], dual):
        assert NEEDS in refused(*off, "--denoise-atrous-slope", "3")
    usage = open(os.path.join(ROOT, "raymond_amd", "host", "cli.cpp")).read().split("#include")[0]  # the usage text is that file's header
    assert "[--denoise-atrous-slope G]" in usage
    undefined = subprocess.run(["nm", "-D", "--undefined-only", cli], check=True, capture_output=True, text=True).stdout
    for name in NEW:
        assert name + "\n" in undefined


# ---------------------------------------------------------------- the restatement's own properties
def _single_frame(W, H):
    halves, F, G, n_f = _frame(W, H)
    return halves[0], halves[1], F, G, halves[4]


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (13, 9)])
def test_the_two_readings_agree_bit_for_bit(W, H):
    S, Q, F, G, n = _single_frame(W, H)
    for levels in (0, 1, 3, 8):
        for slope in (0.0, 3.0):
            a = asref.atrous_slope(S, Q, n, levels=levels, F=F, G=G, slope=slope)
            b = asref.atrous_slope_by_pixel(S, Q, n, levels=levels, F=F, G=G, slope=slope)
            assert a.tobytes() == b.tobytes(), (levels, slope)
    if W * H > 9:  # the slope is not idle on this frame
        assert asref.atrous_slope(S, Q, n, levels=3, F=F, G=G, slope=3.0).tobytes() != asref.atrous_slope(S, Q, n, levels=3, F=F, G=G, slope=0.0).tobytes()


def test_slope_zero_is_the_existing_restatements_bit_for_bit():
    W, H = 13, 9
    S, Q, F, G, n = _single_frame(W, H)
    for kw in (dict(k_f=1.0, tau=1e-2), dict(k_f=0.6, tau=1e-3)):
        for levels in (0, 1, 3, 5):
            a = asref.atrous_slope(S, Q, n, levels=levels, F=F, G=G, slope=0.0, **kw)
            assert a.tobytes() == aref.atrous(S, Q, n, levels=levels, F=F, G=G, **kw).tobytes()
    assert asref.atrous_slope(S, Q, n, levels=3, slope=float("nan")).tobytes() == aref.atrous(S, Q, n, levels=3).tobytes()  # no features: not read
    halves, F, G, n_f = _frame(W, H)
    for levels in (0, 1, 3, 5):
        out, err = asref.atrous_dual_slope(*halves, levels=levels, F=F, G=G, n_f=n_f, slope=0.0)
        want = adref.atrous_dual(*halves, levels=levels, F=F, G=G, n_f=n_f)
        assert out.tobytes() == want[0].tobytes() and err.tobytes() == want[1].tobytes()
    out, err = asref.atrous_dual_slope(*halves, levels=3, slope=7.0)
    want = adref.atrous_dual(*halves, levels=3)
    assert out.tobytes() == want[0].tobytes() and err.tobytes() == want[1].tobytes()


@pytest.mark.parametrize("frame", [gref.step_edge_frame(1), gref.hit_miss_frame()], ids=["step_edge", "hit_miss"])
def test_features_with_a_flat_side_give_the_slope_zero_bytes(frame):
    """A step has a flat side at every pixel, so no slope counts at any level: an edge stays an edge."""
    S, Q, F, G, n = frame[:5]
    zero = asref.atrous_slope(S, Q, n, F=F, G=G, slope=0.0)
    for slope in (1.0, 3.0, 50.0):
        assert asref.atrous_slope(S, Q, n, F=F, G=G, slope=slope).tobytes() == zero.tobytes(), slope
        out, err = asref.atrous_dual_slope(S, Q, S, Q, n, n, F=F, G=G, n_f=n, slope=slope)
        want = asref.atrous_dual_slope(S, Q, S, Q, n, n, F=F, G=G, n_f=n, slope=0.0)
        assert out.tobytes() == want[0].tobytes() and err.tobytes() == want[1].tobytes()
    assert zero.tobytes() != aref.atrous(S, Q, n).tobytes()  # (the guide is not idle)


def test_zero_features_are_the_unguided_bytes():
    S, Q, _, _, n = _single_frame(13, 9)
    n = np.maximum(n, 2)
    Z = np.zeros(n.shape + (7,))
    for levels in (1, 3):
        assert asref.atrous_slope(S, Q, n, levels=levels, F=Z, G=Z, slope=3.0).tobytes() == aref.atrous(S, Q, n, levels=levels).tobytes()


def test_equal_halves_give_the_single_call_and_no_error():
    S, Q, F, G, n = slref.dome_frame(2)[:5]
    for levels in (1, 3):
        single = asref.atrous_slope(S, Q, n, levels=levels, F=F, G=G, slope=3.0)
        out, err = asref.atrous_dual_slope(S, Q, S, Q, n, n, levels=levels, F=F, G=G, n_f=n, slope=3.0)
        assert out.tobytes() == single.tobytes() and np.all(err == 0.0)  # (n + n is a power of two times n: the combination is exact)
    assert single.tobytes() != asref.atrous_slope(S, Q, n, levels=3, F=F, G=G, slope=0.0).tobytes()


REGIONS = {"one": [(19, 11, 5, 3)], "corners": [(0, 0, 6, 4), (41, 27, 7, 5)], "quarters": [(0, 0, 24, 16), (24, 0, 24, 16), (0, 16, 24, 16), (24, 16, 24, 16)]}


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_the_region_restatement_is_the_whole_frame_inside_the_region(levels):
    """The floors are made from the f of the prologue's set and kept on level 0's set alone — NaN denominators everywhere else —, and every region
    pixel still gets the whole frame's bytes: the existing needed sets carry the slope too.  A dome (the slope matters) with planted bad pixels."""
    S, Q, F, G, n = slref.dome_frame(3)[:5]
    rng = np.random.default_rng(5)
    Sb, Qb = S + rng.normal(0, 0.3, S.shape), Q + rng.normal(0, 0.3, S.shape) ** 2
    F, G = F.copy(), G.copy()
    F[10, 20, 4], G[16, 30, 6] = np.nan, np.inf
    n_f = 2 * n
    n_f[5, 17] = 1
    out_x, err_x = asref.atrous_dual_slope(S, Q, Sb, Qb, n, n, levels=levels, F=2 * F, G=2 * G, n_f=n_f, slope=3.0)
    zero = asref.atrous_dual_slope(S, Q, Sb, Qb, n, n, levels=levels, F=2 * F, G=2 * G, n_f=n_f, slope=0.0)[0]
    assert not np.array_equal(out_x, zero, equal_nan=True)
    for name, region in REGIONS.items():
        out, err = asref.atrous_dual_slope_region(S, Q, Sb, Qb, n, n, region, levels=levels, F=2 * F, G=2 * G, n_f=n_f, slope=3.0)
        inside = asref.rref.region_mask(region, 48, 32)
        assert out[inside].tobytes() == out_x[inside].tobytes() and err[inside].tobytes() == err_x[inside].tobytes(), name
        assert np.isnan(out[~inside]).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_dome(seed):
    """Flat colour under a dome of normals, 5 levels, k 3, k_f 1, tau 1e-2 (the defaults): at slope 0 the guided filter loses every level but the first
    to the normal term.  Disc RMSE at slope 3 is below 0.5 of slope 0's (computed for the issue on this restatement's operations: 0.34 - 0.37), and at
    slope 8 below slope 3's — a larger slope opens more levels."""
    S, Q, F, G, n, truth, disc = slref.dome_frame(seed)
    r = {s: slref.disc_rmse(asref.atrous_slope(S, Q, n, F=F, G=G, slope=s), truth, disc) for s in (0.0, 3.0, 8.0)}
    un = slref.disc_rmse(aref.atrous(S, Q, n), truth, disc)
    print("dome seed %d: disc RMSE unguided %.5f slope 0 %.5f slope 3 %.5f (x%.3f) slope 8 %.5f" % (seed, un, r[0.0], r[3.0], r[3.0] / r[0.0], r[8.0]))
    assert r[3.0] < 0.5 * r[0.0]
    assert r[8.0] < r[3.0]


# ---------------------------------------------------------------- the scratch block
@pytest.mark.parametrize("form", ["atrous", "atrous_dual", "atrous_dual_region"])
def test_the_slope_planes_exist_only_with_a_slope_and_lie_behind_everything_else(form):
    for (W, H), n_rects, n_table in (((1, 1), 0, 0), ((37, 23), 3, 0), ((45, 29), 1, 5)):
        N = W * H
        before = probe.denoise_scratch(form, W, H, n_rects, True, 0, n_table)
        off = probe.denoise_scratch(form, W, H, n_rects, True, 0, n_table, atrous_sloped=False)
        on = probe.denoise_scratch(form, W, H, n_rects, True, 0, n_table, atrous_sloped=True)
        assert off == before and "slope_planes" not in off[0]  # slope 0: the block of the call without the suffix
        parts, total = on
        assert set(parts) == set(before[0]) | {"slope_planes"}
        assert all(parts[k] == before[0][k] for k in before[0])  # every existing part where it was, as long as it was
        assert parts["slope_planes"] == (before[1], 8 * 7 * N) and before[1] % 16 == 0  # behind everything else
        assert total == before[1] + (8 * 7 * N + 15) // 16 * 16
        # without features there is nothing to take a slope of
        assert probe.denoise_scratch(form, W, H, n_rects, False, 0, n_table, atrous_sloped=True) == probe.denoise_scratch(form, W, H, n_rects, False, 0, n_table)


@pytest.mark.parametrize("form", ["single", "dual", "dual_select", "tile_error"])
def test_the_other_forms_do_not_answer_to_the_atrous_slope(form):
    guided = form != "tile_error"
    n_cands = 2 if form == "dual_select" else 0
    assert probe.denoise_scratch(form, 37, 23, 3, guided, n_cands, 5, atrous_sloped=True) == probe.denoise_scratch(form, 37, 23, 3, guided, n_cands, 5)
