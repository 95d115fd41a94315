"""rmd_denoise_dual_guided and rmd_denoise_dual_guided_region: the parts that need no GPU.

The entry points are exported and declared as the header states them, every argument rule holds before a device is touched, the Python Settings
accept and refuse what they should, and the numpy restatement (tests/denoise_dual_guided_ref.py) agrees with a per-pixel-loop reading of the
definition and keeps the definition's exact identities.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_dual_guided_ref as dgref
import denoise_dual_ref
import denoise_guided_ref as gref
import denoise_ref
from raymond_amd import abi, lib, scenes
from raymond_amd.scene import Settings
from test_denoise_dual_host import _half, _two_halves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
NEW = ("rmd_denoise_dual_guided", "rmd_denoise_dual_guided_region")
PARAMS = dict(radius=10, patch_radius=3, k=0.45, alpha=1.0, k_f=1.0, tau=1e-2)  # the issue's


# ---------------------------------------------------------------- the boundary
def test_guided_dual_entry_points_are_exported_and_declared(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    for name in NEW:
        assert name in exported and name in lib.SIGNATURES and "rmd_status " + name + "(" in header
        assert name in open(os.path.join(ROOT, "integration", "gpu.rs")).read()
    n_args = {name: len(lib.SIGNATURES[name][1]) for name in NEW + ("rmd_denoise_dual", "rmd_denoise_dual_region")}
    assert n_args == {"rmd_denoise_dual_guided": 22, "rmd_denoise_dual_guided_region": 24, "rmd_denoise_dual": 17, "rmd_denoise_dual_region": 19}
    for name, n in n_args.items():  # the header's declarations have as many parameters
        decl = re.search(r"rmd_status " + name + r"\(([^)]*)\);", header).group(1)
        assert len(decl.split(",")) == n, name
    assert ("rmd_status rmd_denoise_dual_guided(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev, "
            "const double *accum_sq_b_dev, const double *feat_dev, const double *feat_sq_dev, uint32_t width, uint32_t height, "
            "const rmd_tile_rect *rects, const uint32_t *rect_counts_a, const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects, "
            "uint32_t radius, uint32_t patch_radius, double k, double alpha, double k_f, double tau, double *out_dev, double *err_dev);") in header
    assert ("const uint32_t *rect_counts_f, uint32_t n_rects, const rmd_tile_rect *region, uint32_t n_region, uint32_t radius, uint32_t patch_radius, "
            "double k, double alpha, double k_f, double tau, double *out_dev, double *err_dev);") in header
    assert "#define RMD_ABI_VERSION 6u" in header  # additions within ABI 6
    fault_list = header[header.index("RMD_ERR_DEVICE_FAULT = 8") : header.index("};", header.index("RMD_ERR_DEVICE_FAULT = 8"))]
    assert "rmd_denoise_dual_guided," in fault_list and "rmd_denoise_dual_guided_region" in fault_list  # both wait, both report an earlier fault


def _last_error(L):
    return (L.rmd_last_error(None) or b"").decode()


def _rects(*rs):
    arr = (abi.TileRect * max(1, len(rs)))()
    for i, (l, t, w, h) in enumerate(rs):
        arr[i].left, arr[i].top, arr[i].width, arr[i].height = l, t, w, h
    return arr


@pytest.mark.parametrize("regional", [False, True])
def test_guided_dual_argument_rules_without_a_device(product_lib, regional):
    """Every bad argument is RMD_ERR_INVALID_ARGUMENT with its own message before the context is looked at; good ones reach 'null context'."""
    L = product_lib
    W, H = 8, 8
    span, fspan = W * H * 3 * 8, W * H * 7 * 8
    base = 0x100000
    sa, qa, sb, qb, o = (C.c_void_p(base + i * span) for i in range(5))
    e = C.c_void_p(base + 5 * span)
    fbase = base + 6 * span
    ft, gt = C.c_void_p(fbase), C.c_void_p(fbase + fspan)
    full = _rects((0, 0, 8, 8))
    counts = (C.c_uint32 * 2)(4, 4)

    def call(SA=sa, QA=qa, SB=sb, QB=qb, F=ft, G=gt, w=W, h=H, rects=full, ca=counts, cb=counts, cf=counts, n_rects=1, region=full, n_region=1, r=10, f=3,
             k=0.45, alpha=1.0, k_f=1.0, tau=1e-2, out=o, err=e):
        if regional:
            return L.rmd_denoise_dual_guided_region(None, SA, QA, SB, QB, F, G, w, h, rects, ca, cb, cf, n_rects, region, n_region, r, f, k, alpha, k_f, tau,
                                                    out, err)
        return L.rmd_denoise_dual_guided(None, SA, QA, SB, QB, F, G, w, h, rects, ca, cb, cf, n_rects, r, f, k, alpha, k_f, tau, out, err)

    def refused(word, **kw):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert word in _last_error(L), (kw, _last_error(L))
        assert _last_error(L).startswith("rmd_denoise_dual_guided_region: " if regional else "rmd_denoise_dual_guided: ")

    # every rule of rmd_denoise_dual[_region]
    for name in ("SA", "QA", "SB", "QB", "out", "rects", "ca", "cb"):
        refused("bad argument", **{name: None})
    refused("bad argument", w=0)
    refused("bad argument", h=0)
    names = ["SA", "QA", "SB", "QB", "out", "err"]
    ptrs = [sa, qa, sb, qb, o, e]
    for i in range(6):
        for j in range(6):
            if i != j:
                refused("alias", **{names[i]: ptrs[j]})
    refused("alias", err=C.c_void_p(base + 5 * span - 8))
    refused("alias", err=C.c_void_p(base - W * H * 8 + 8))
    refused("radius", r=13)
    refused("patch_radius", f=5)
    for k in (0.0, -0.45, float("nan"), float("inf")):
        refused("k must", k=k)
    for a in (-1e-300, float("nan"), float("inf")):
        refused("alpha", alpha=a)
    refused("outside", rects=_rects((0, 0, 9, 8)))
    refused("overlap", rects=_rects((0, 0, 4, 4), (3, 3, 2, 2)), n_rects=2)
    if regional:
        refused("region is NULL", region=None)
        refused("region: tile rectangle outside", region=_rects((0, 0, 9, 8)))
        refused("region: tile rectangles overlap", region=_rects((0, 0, 4, 4), (3, 3, 2, 2)), n_region=2)
    # the feature rules
    refused("both be given or both be NULL", F=None)
    refused("both be given or both be NULL", G=None)
    refused("rect_counts_f", cf=None)
    for v in (0.0, -1.0, float("nan"), float("inf")):
        refused("k_f must", k_f=v)
        refused("tau must", tau=v)
    refused("feat_dev and feat_sq_dev must not alias", G=ft)
    refused("feat_dev and feat_sq_dev must not alias", G=C.c_void_p(fbase + fspan - 8))
    for p in ptrs:  # either feature range on any of the six
        refused("feat_dev and feat_sq_dev must not alias", F=p)
        refused("feat_dev and feat_sq_dev must not alias", G=p)
    refused("feat_dev and feat_sq_dev must not alias", F=C.c_void_p(base + 5 * span + W * H * 8 - 8))  # its first double is err_dev's last
    refused("feat_dev and feat_sq_dev must not alias", G=C.c_void_p(base - fspan + 8))  # its last double is accum_a_dev's first
    # good arguments get as far as the context
    good = [{}, dict(r=12, f=4), dict(r=0, f=0), dict(err=None), dict(rects=None, ca=None, cb=None, cf=None, n_rects=0),
            dict(G=C.c_void_p(base - fspan)),  # directly in front of accum_a_dev
            dict(F=None, G=None), dict(F=None, G=None, cf=None, k_f=float("nan"), tau=-1.0)]  # no features: rect_counts_f, k_f and tau are not read
    if regional:
        good += [dict(region=None, n_region=0), dict(region=_rects((1, 1, 3, 5), (5, 0, 3, 3)), n_region=2)]
    for kw in good:
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert _last_error(L) == "null context", (kw, _last_error(L))


def test_settings_dual_features_rules():
    cam = scenes.camera(64, 64)
    assert Settings(cam, 16).denoise_dual_features is False
    st = Settings(cam, 64, denoise=True, denoise_dual=True, denoise_dual_features=True, samples_per_iteration=8)
    assert st.denoise_dual_features and (st.denoise_feature_k, st.denoise_feature_tau) == (1.0, 1e-2)
    Settings(cam, 64, denoise=True, denoise_dual=True, denoise_dual_features=True, samples_per_iteration=8, adaptive_denoised_threshold=0.01,
             denoise_feature_k=0.6, denoise_feature_tau=1e-3)
    with pytest.raises(ValueError, match="denoise_dual_features needs denoise_dual"):
        Settings(cam, 64, denoise=True, denoise_dual_features=True, samples_per_iteration=8)
    with pytest.raises(ValueError):
        Settings(cam, 64, denoise_dual_features=True)
    for bad in (dict(denoise_feature_k=0.0), dict(denoise_feature_tau=float("nan"))):  # check_denoise validates what the guided call reads
        with pytest.raises(ValueError):
            Settings(cam, 64, denoise=True, denoise_dual=True, denoise_dual_features=True, samples_per_iteration=8, **bad)
    with pytest.raises(ValueError, match="denoise_features"):  # as before: the old pair stays refused, with or without the new setting
        Settings(cam, 64, denoise=True, denoise_dual=True, samples_per_iteration=8, denoise_features=True)
    with pytest.raises(ValueError, match="denoise_features"):
        Settings(cam, 64, denoise=True, denoise_dual=True, denoise_dual_features=True, samples_per_iteration=8, denoise_features=True)


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


def test_cli_dual_features_rules(cli, tmp_path):
    """render_tiled (C++) throws raymond::Error before it starts a worker: no device is needed to see it."""
    r = subprocess.run([cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm"), "--denoise", "1", "--spi", "4", "--denoise-dual-features", "1"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "denoise_dual_features needs denoise_dual" in r.stderr, r.stderr
    r = subprocess.run([cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm"), "--denoise", "1", "--spi", "4", "--denoise-dual", "1",
                        "--denoise-dual-features", "1", "--denoise-features", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and "denoise_features" in r.stderr, r.stderr
    usage = open(os.path.join(ROOT, "raymond_amd", "host", "cli.cpp")).read().split("#include")[0]  # the usage text is that file's header
    assert "[--denoise-dual-features 1]" in usage


# ---------------------------------------------------------------- the restatement's own properties
def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _features(rng, H, W, n_f):
    """Random feature sums and sums of squares at n_f (H, W) samples, with a NaN, an inf and counts of 0 and 1 among them."""
    nd = np.maximum(n_f, 1).astype(np.float64)[..., None]
    f = rng.uniform(-1.0, 1.0, (H, W, 7)) * np.array([1, 1, 1, 1, 1, 1, 5.0])
    F = f * nd
    G = F * f + rng.uniform(0.0, 0.05, (H, W, 7)) * np.maximum(nd - 1.0, 0.0)
    return F, G


@pytest.mark.parametrize("r,f,k_f,tau", [(0, 0, 1.0, 1e-2), (1, 0, 1.0, 1e-2), (2, 1, 0.6, 1e-3), (3, 2, 1.0, 1e-2)])
def test_restatement_agrees_with_the_per_pixel_reading(r, f, k_f, tau):
    """As denoise_dual_ref is held to denoise_dual_naive: the same operations in the same order; numpy's exp of an array and of a scalar may differ
    in the last bit, hence 4 ulp on a weighted mean."""
    H, W = 7, 9
    halves = _two_halves(11, H, W)
    rng = np.random.default_rng(111)
    n_f = rng.integers(2, 40, (H, W))
    n_f[0, 0], n_f[6, 8] = 0, 1
    F, G = _features(rng, H, W, n_f)
    F[2, 2, 4], G[5, 1, 6] = np.nan, np.inf
    out, err = dgref.denoise_dual_guided(*halves, F, G, n_f, radius=r, patch_radius=f, k=0.45, alpha=1.0, k_f=k_f, tau=tau)
    out_n, err_n = dgref.denoise_dual_guided_naive(*halves, F, G, n_f, r, f, 0.45, 1.0, k_f, tau)
    assert np.array_equal(np.isnan(out), np.isnan(out_n)) and np.array_equal(np.isnan(err), np.isnan(err_n))
    assert np.isnan(err).sum() == 5  # the five pixels that are not dual-valid
    fin = np.isfinite(out_n)
    assert np.all(np.abs(out[fin] - out_n[fin]) <= 4 * np.spacing(np.abs(out_n[fin])))
    fin = np.isfinite(err_n)
    assert np.allclose(err[fin], err_n[fin], rtol=1e-9, atol=1e-30)
    if r > 0:  # the features do something on this input
        un, _ = denoise_dual_ref.denoise_dual(*halves, radius=r, patch_radius=f)
        assert not _same(out, un)


@pytest.mark.parametrize("r,f", [(1, 0), (3, 1), (5, 2)])
def test_restatement_equal_halves_give_rmd_denoise_guided_and_no_error(r, f):
    """Identity 1: A == B with the features' counts equal to the half's: f_A == f_B == denoise_guided(half) bit for bit and err == 0."""
    rng = np.random.default_rng(13)
    H, W, n = 12, 15, 8
    n_img = np.full((H, W), n)
    n_img[5, 5] = 1  # a pixel that is not valid in either half
    S, Q = _half(rng, H, W, n_img)
    F, G = _features(rng, H, W, n_img)
    F[3, 3, 0] = np.nan  # valid, not feature-valid
    f_a, f_b, dual = dgref.filtered_halves(S, Q, S, Q, n_img, n_img, F, G, n_img, radius=r, patch_radius=f)
    single = gref.denoise_guided(S, Q, F, G, n_img, radius=r, patch_radius=f, k_f=1.0, tau=1e-2)
    assert not dual[5, 5] and dual.sum() == H * W - 1
    assert f_a[dual].tobytes() == f_b[dual].tobytes() == single[dual].tobytes()
    out, err = dgref.denoise_dual_guided(S, Q, S, Q, n_img, n_img, F, G, n_img, radius=r, patch_radius=f)
    assert out[dual].tobytes() == single[dual].tobytes()  # (n f + n f) / (2 n) is f again at a power of two
    assert np.isnan(err[5, 5]) and np.all(err[dual] == 0.0)
    plain = denoise_ref.denoise(S, Q, n_img, radius=r, patch_radius=f)
    assert not _same(single, plain)


@pytest.mark.parametrize("r,f", [(3, 1), (10, 3)])
def test_restatement_zero_or_absent_features_give_denoise_dual(r, f):
    """Identities 2 and 3, bit for bit, NaN where denoise_dual has NaN."""
    H, W = 23, 37
    halves = _two_halves(17, H, W)
    want = denoise_dual_ref.denoise_dual(*halves, radius=r, patch_radius=f)
    Z = np.zeros((H, W, 7))
    n_f = np.full((H, W), 5)
    zero = dgref.denoise_dual_guided(*halves, Z, Z, n_f, radius=r, patch_radius=f)
    none = dgref.denoise_dual_guided(*halves, None, None, None, radius=r, patch_radius=f)
    for got in (zero, none):
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert np.isnan(want[1]).any() and np.isfinite(want[1]).any()


def test_restatement_hit_miss_frame_comes_back_exact():
    S, Q, F, G, n, u = gref.hit_miss_frame()
    out, err = dgref.denoise_dual_guided(S, Q, S, Q, n, n, F + F, G + G, n + n, **PARAMS)
    assert out.tobytes() == u.tobytes() and np.all(err == 0.0)
    un, _ = denoise_dual_ref.denoise_dual(S, Q, S, Q, n, n)
    assert np.abs(un - u).max() > 0.2  # the colour weights alone mix across the step


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_restatement_keeps_a_step_edge_below_the_noise(seed):
    """Halves step_edge_frame(seed) and (seed + 1000), the features of A added to themselves at a count of 32.  The prototype gave 0.21 - 0.31; the
    bar is the issue's 0.5."""
    S_a, Q_a, F, G, n, truth = gref.step_edge_frame(seed)
    S_b, Q_b = gref.step_edge_frame(seed + 1000)[:2]
    gd, err_g = dgref.denoise_dual_guided(S_a, Q_a, S_b, Q_b, n, n, F + F, G + G, n + n, **PARAMS)
    un, err_u = denoise_dual_ref.denoise_dual(S_a, Q_a, S_b, Q_b, n, n, radius=10, patch_radius=3, k=0.45, alpha=1.0)
    rg, ru = gref.band_rmse(gd, truth), gref.band_rmse(un, truth)
    print("step edge seed %d: band RMSE guided dual %.5f denoise_dual %.5f ratio %.3f; sqrt(mean err) %.5f / %.5f" %
          (seed, rg, ru, rg / ru, np.sqrt(err_g.mean()), np.sqrt(err_u.mean())))
    assert rg <= 0.5 * ru
