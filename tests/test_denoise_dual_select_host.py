"""rmd_denoise_dual_select: the parts that need no GPU.

The entry point is exported and declared as the header states it, the candidate struct has the header's layout, every argument rule holds before a
device is touched, the Python Settings and the CLI accept and refuse what they should, and the numpy restatement (tests/denoise_dual_select_ref.py)
agrees with a per-pixel-loop reading of the definition and keeps the definition's two consequences: one candidate is denoise_dual_guided_ref, and a
candidate listed twice changes nothing.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_dual_guided_ref as dgref
import denoise_dual_select_ref as sref
from raymond_amd import abi, lib, scenes
from raymond_amd.scene import Settings
from test_denoise_dual_guided_host import _features, _last_error, _rects
from test_denoise_dual_host import _half, _two_halves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
NAME = "rmd_denoise_dual_select"


# ---------------------------------------------------------------- the boundary
def test_select_entry_point_is_exported_and_declared(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert NAME in set(re.findall(r" T (\w+)", out))
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    assert ("rmd_status rmd_denoise_dual_select(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev, "
            "const double *accum_sq_b_dev, const double *feat_dev, const double *feat_sq_dev, uint32_t width, uint32_t height, "
            "const rmd_tile_rect *rects, const uint32_t *rect_counts_a, const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects, "
            "uint32_t radius, uint32_t patch_radius, const rmd_denoise_candidate *cands, uint32_t n_cands, uint32_t sure_window, uint32_t select_window, "
            "double *out_dev, double *err_dev, double *sure_dev, uint32_t *win_dev);") in header
    assert len(lib.SIGNATURES[NAME][1]) == 24
    assert "#define RMD_ABI_VERSION 6u" in header  # an addition within ABI 6
    fault_list = header[header.index("RMD_ERR_DEVICE_FAULT = 8") : header.index("};", header.index("RMD_ERR_DEVICE_FAULT = 8"))]
    assert NAME in fault_list
    rs = open(os.path.join(ROOT, "integration", "gpu.rs")).read()
    assert NAME in rs and "rmd_denoise_candidate" in rs
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_candidate_struct_layout_matches_the_header():
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    assert "typedef struct rmd_denoise_candidate { double k, alpha, k_f, tau; uint32_t guided, reserved; } rmd_denoise_candidate;" in header
    assert "enum { RMD_DENOISE_MAX_CANDIDATES = 4 };" in header and abi.DENOISE_MAX_CANDIDATES == 4
    S = abi.DenoiseCandidate
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == [("k", 0, 8), ("alpha", 8, 8), ("k_f", 16, 8), ("tau", 24, 8),
                                                                                      ("guided", 32, 4), ("reserved", 36, 4)]
    assert C.sizeof(S) == 40 and C.alignment(S) == 8


def _cands(*cs):
    arr = (abi.DenoiseCandidate * max(1, len(cs)))()
    for i, c in enumerate(cs):
        arr[i] = abi.DenoiseCandidate(c.get("k", 0.45), c.get("alpha", 1.0), c.get("k_f", 1.0), c.get("tau", 1e-2), c.get("guided", 0), c.get("reserved", 0))
    return arr


def test_select_argument_rules_without_a_device(product_lib):
    """Every bad argument is RMD_ERR_INVALID_ARGUMENT with its own message before the context is looked at; good ones reach 'null context'."""
    L = product_lib
    W, H = 8, 8
    span, fspan = W * H * 3 * 8, W * H * 7 * 8
    base = 0x100000
    sa, qa, sb, qb, o = (C.c_void_p(base + i * span) for i in range(5))
    e, su, wi = C.c_void_p(base + 5 * span), C.c_void_p(base + 5 * span + W * H * 8), C.c_void_p(base + 5 * span + 2 * W * H * 8)
    fbase = base + 6 * span
    ft, gt = C.c_void_p(fbase), C.c_void_p(fbase + fspan)
    full = _rects((0, 0, 8, 8))
    counts = (C.c_uint32 * 2)(4, 4)
    two = _cands(dict(k=0.45), dict(k=1.0, guided=1))

    def call(SA=sa, QA=qa, SB=sb, QB=qb, F=ft, G=gt, w=W, h=H, rects=full, ca=counts, cb=counts, cf=counts, n_rects=1, r=10, f=3, cands=two, n=2, sw=2, lw=2,
             out=o, err=e, sure=su, win=wi):
        return L.rmd_denoise_dual_select(None, SA, QA, SB, QB, F, G, w, h, rects, ca, cb, cf, n_rects, r, f, cands, n, sw, lw, out, err, sure, win)

    def refused(word, **kw):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert word in _last_error(L), (kw, _last_error(L))
        assert _last_error(L).startswith("rmd_denoise_dual_select: ")

    # rmd_denoise_dual's rules
    for name in ("SA", "QA", "SB", "QB", "out", "rects", "ca", "cb"):
        refused("bad argument", **{name: None})
    refused("bad argument", w=0)
    refused("bad argument", h=0)
    names = ["SA", "QA", "SB", "QB", "out", "err", "sure", "win"]
    ptrs = [sa, qa, sb, qb, o, e, su, wi]
    for i in range(8):
        for j in range(8):
            if i != j:
                refused("alias", **{names[i]: ptrs[j]})
    refused("alias", sure=C.c_void_p(base + 5 * span + 8))  # into err_dev
    refused("alias", win=C.c_void_p(base - W * H * 4 + 4))  # its last word is accum_a_dev's first
    refused("alias", F=sa)
    refused("alias", G=C.c_void_p(fbase + fspan - 8))
    refused("radius", r=13)
    refused("patch_radius", f=5)
    refused("outside", rects=_rects((0, 0, 9, 8)))
    refused("overlap", rects=_rects((0, 0, 4, 4), (3, 3, 2, 2)), n_rects=2)
    # the rules of its own
    refused("n_cands", n=0)
    refused("n_cands", n=5, cands=_cands(*[dict()] * 5))
    refused("n_cands", cands=None)
    refused("sure_window and select_window", sw=6)
    refused("sure_window and select_window", lw=6)
    refused("reserved", cands=_cands(dict(), dict(reserved=1)))
    refused("candidate 1: guided", F=None, G=None)
    refused("both be given or both be NULL", F=None)
    refused("both be given or both be NULL", G=None)
    refused("rect_counts_f", cf=None)
    for v in (0.0, -0.45, float("nan"), float("inf")):
        refused("candidate 0: k must", cands=_cands(dict(k=v), dict(guided=1)))
        refused("candidate 1: k must", cands=_cands(dict(), dict(k=v)))
        refused("candidate 1: k_f must", cands=_cands(dict(), dict(guided=1, k_f=v)))
        refused("candidate 1: tau must", cands=_cands(dict(), dict(guided=1, tau=v)))
    for a in (-1e-300, float("nan"), float("inf")):
        refused("candidate 0: alpha", cands=_cands(dict(alpha=a), dict(guided=1)))
    # good arguments get as far as the context
    good = [{}, dict(r=12, f=4, sw=5, lw=5), dict(r=0, f=0, sw=0, lw=0), dict(err=None), dict(sure=None), dict(win=None), dict(err=None, sure=None, win=None),
            dict(rects=None, ca=None, cb=None, cf=None, n_rects=0), dict(n=1), dict(n=4, cands=_cands(*[dict(guided=i & 1) for i in range(4)])),
            dict(F=None, G=None, cf=None, cands=_cands(dict(), dict(k=1.0, k_f=float("nan"), tau=-1.0))),  # unguided: k_f and tau are not read
            dict(cf=None, cands=_cands(dict(), dict(k=1.0)))]  # features given, no guided candidate: they and rect_counts_f are not read
    for kw in good:
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert _last_error(L) == "null context", (kw, _last_error(L))


def test_settings_dual_select_rules():
    cam = scenes.camera(64, 64)
    assert Settings(cam, 16).denoise_dual_select is False
    st = Settings(cam, 64, denoise=True, denoise_dual=True, denoise_dual_select=True, samples_per_iteration=8, denoise_k=0.5, denoise_feature_k=0.8)
    assert st.denoise_dual_select and not st.denoise_dual_features
    assert st.select_candidates() == [dict(k=0.5, alpha=1.0), dict(k=1.0, alpha=1.0, guided=True, k_f=0.8, tau=1e-2)]
    Settings(cam, 64, denoise=True, denoise_dual=True, denoise_dual_select=True, denoise_dual_features=True, samples_per_iteration=8, adaptive_denoised_threshold=0.01)
    with pytest.raises(ValueError, match="denoise_dual_select needs denoise_dual"):
        Settings(cam, 64, denoise=True, denoise_dual_select=True, samples_per_iteration=8)
    with pytest.raises(ValueError):
        Settings(cam, 64, denoise_dual_select=True)
    for bad in (dict(denoise_feature_k=0.0), dict(denoise_feature_tau=float("nan")), dict(denoise_k=-1.0)):
        with pytest.raises(ValueError):
            Settings(cam, 64, denoise=True, denoise_dual=True, denoise_dual_select=True, samples_per_iteration=8, **bad)


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


def test_cli_dual_select_rules(cli, tmp_path):
    """render_tiled (C++) throws raymond::Error before it starts a worker: no device is needed to see it."""
    r = subprocess.run([cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm"), "--denoise", "1", "--spi", "4", "--denoise-dual-select", "1"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "denoise_dual_select needs denoise_dual" in r.stderr, r.stderr
    usage = open(os.path.join(ROOT, "raymond_amd", "host", "cli.cpp")).read().split("#include")[0]  # the usage text is that file's header
    assert "[--denoise-dual-select 1]" in usage
    undefined = subprocess.run(["nm", "-D", "--undefined-only", cli], check=True, capture_output=True, text=True).stdout
    assert "rmd_denoise_dual_select" in undefined


# ---------------------------------------------------------------- the restatement
def _frame(W, H, seed=11):
    """Two halves, features and their counts on a W x H frame; from 5 x 5 up with test_denoise_dual_host's planted pixels that are not dual-valid."""
    rng = np.random.default_rng(1000 * W + H)
    if W >= 5 and H >= 5:
        halves = _two_halves(seed, H, W)
    else:
        n_a, n_b = rng.integers(2, 20, (H, W)), rng.integers(2, 20, (H, W))
        halves = (*_half(rng, H, W, n_a), *_half(rng, H, W, n_b), n_a, n_b)
    n_f = rng.integers(2, 40, (H, W))
    if W >= 5 and H >= 5:
        n_f[0, 0], n_f[H - 1, W - 1] = 0, 1
    F, G = _features(rng, H, W, n_f)
    if W >= 5 and H >= 5:
        F[2, 2, 4], G[4, 1, 6] = np.nan, np.inf
    return halves, F, G, n_f


CANDS = [dict(k=0.45, alpha=1.0), dict(k=1.0, alpha=1.0, guided=True, k_f=1.0, tau=1e-2), dict(k=0.3, alpha=0.5, guided=True, k_f=0.6, tau=1e-3)]


@pytest.mark.parametrize("sw,lw", [(0, 0), (1, 2), (2, 2), (2, 0)])
@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (13, 9)])
def test_restatement_agrees_with_the_per_pixel_reading(W, H, sw, lw):
    """The same operations in the same order; numpy's exp of an array and of a scalar may differ in the last bit, so the per-pixel reading's winners
    are required wherever the vectorised form's two smallest window means are not within 1e-9 of each other, and the values are compared with the
    vectorised form blending by the per-pixel reading's winners."""
    halves, F, G, n_f = _frame(W, H)
    r, f = 2, 1
    naive = sref.denoise_dual_select_naive(*halves, CANDS, F, G, n_f, r, f, sw, lw)
    own = sref.denoise_dual_select(*halves, CANDS, F, G, n_f, radius=r, patch_radius=f, sure_window=sw, select_window=lw)
    dual = own["dual"]
    assert np.array_equal(naive["win"] == sref.NO_WINNER, ~dual)
    tie = sref.near_ties(own["E"], dual)
    assert np.array_equal(naive["win"][~tie], own["own_win"][~tie]) and tie.sum() <= 0.05 * dual.sum()
    got = sref.denoise_dual_select(*halves, CANDS, F, G, n_f, radius=r, patch_radius=f, sure_window=sw, select_window=lw, win=naive["win"], parts=own["parts"])
    for name in ("out", "err", "sure"):
        a, b = got[name], naive[name]
        assert np.array_equal(np.isnan(a), np.isnan(b)), name
        fin = np.isfinite(b)
        scale = np.max(np.abs(b[fin])) if fin.any() else 0.0
        assert np.all(np.abs(a[fin] - b[fin]) <= 1e-12 * np.abs(b[fin]) + 1e-14 * scale), name
    if W * H > 1:
        assert np.isnan(own["sure"]).sum() == (~dual).sum() > 0 and len(set(own["own_win"][dual].tolist())) >= 2  # more than one candidate wins somewhere


@pytest.mark.parametrize("cand", [CANDS[0], CANDS[1], CANDS[2]])
def test_restatement_with_one_candidate_is_denoise_dual_guided_ref(cand):
    W, H = 13, 9
    halves, F, G, n_f = _frame(W, H)
    k, alpha, guided, k_f, tau = sref._cand(cand)
    got = sref.denoise_dual_select(*halves, [cand], F, G, n_f, radius=3, patch_radius=1, sure_window=2, select_window=2)
    feats = (F, G, n_f) if guided else (None, None, None)
    out, err = dgref.denoise_dual_guided(*halves, *feats, radius=3, patch_radius=1, k=k, alpha=alpha, k_f=k_f, tau=tau)
    assert got["out"].tobytes() == out.tobytes() and got["err"].tobytes() == err.tobytes()
    assert np.all(got["win"][got["dual"]] == 0) and np.all(got["win"][~got["dual"]] == sref.NO_WINNER)
    assert np.isnan(err).any() and np.isfinite(err).any()


@pytest.mark.parametrize("sw,lw", [(0, 0), (2, 2)])
def test_restatement_with_a_duplicated_candidate_is_unchanged(sw, lw):
    W, H = 13, 9
    halves, F, G, n_f = _frame(W, H)
    kw = dict(radius=3, patch_radius=1, sure_window=sw, select_window=lw)
    once = sref.denoise_dual_select(*halves, CANDS[:2], F, G, n_f, **kw)
    twice = sref.denoise_dual_select(*halves, [CANDS[0], CANDS[1], CANDS[0], CANDS[1]], F, G, n_f, **kw)
    for name in ("out", "err", "sure", "win"):
        assert once[name].tobytes() == twice[name].tobytes(), name
    same = sref.denoise_dual_select(*halves, [CANDS[1], CANDS[1]], F, G, n_f, **kw)
    alone = sref.denoise_dual_select(*halves, [CANDS[1]], F, G, n_f, **kw)
    assert np.all(same["win"][same["dual"]] == 0) and same["out"].tobytes() == alone["out"].tobytes() and same["sure"].tobytes() == alone["sure"].tobytes()


def test_restatement_radius_zero_is_the_closed_form():
    """r = 0: one neighbour, w = 1, g = 1, f = u: sure_X is the mean of v_X over the channels, exactly."""
    W, H = 13, 9
    halves, F, G, n_f = _frame(W, H)
    planes = sref._planes(*halves)
    f_a, f_b, sure = sref.candidate(planes, halves[4], halves[5], CANDS[1], F, G, n_f, 0, 2)
    u_a, v_a, u_b, v_b, dual = planes
    na, nb = halves[4].astype(np.float64), halves[5].astype(np.float64)
    with np.errstate(all="ignore"):
        sx = [((0.0 - v[..., 0]) + 2.0 * v[..., 0] + ((0.0 - v[..., 1]) + 2.0 * v[..., 1]) + ((0.0 - v[..., 2]) + 2.0 * v[..., 2])) / 3.0 for v in (v_a, v_b)]
        want = (na * sx[0] + nb * sx[1]) / (na + nb)
    assert f_a[dual].tobytes() == u_a[dual].tobytes() and f_b[dual].tobytes() == u_b[dual].tobytes()
    assert sure[dual].tobytes() == want[dual].tobytes() and np.isnan(sure[~dual]).all()
