"""First-hit feature buffers and rmd_denoise_guided: the parts that need no GPU.

The numpy restatement (tests/denoise_guided_ref.py) keeps the exact properties of the definition, the entry points are exported and declared,
their argument rules hold before a device is touched, and the Python Settings refuse bad feature settings.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_guided_ref as gref
import denoise_ref
import test_gpu_denoise as tgd
from raymond_amd import abi, lib, scenes
from raymond_amd.scene import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rmd_feature_buffer_alloc", "rmd_render_features", "rmd_render_features_async", "rmd_denoise_guided")


# ---------------------------------------------------------------- the restatement's own properties
@pytest.mark.parametrize("r,f", [(3, 1), (10, 3)])
def test_zero_features_are_the_unguided_filter_bit_for_bit(r, f):
    rng = np.random.default_rng(37023)
    W, H = 37, 23
    rects, counts = tgd._tiles_with_counts(W, H, 8, 16, rng)  # counts include 0 and 1, and one tile is left out
    n_img = denoise_ref.count_image(W, H, rects, counts)
    S, Q = tgd._moments(rng, n_img)
    tgd._poison(S, Q, rng)
    Z = np.zeros((H, W, 7))
    a = denoise_ref.denoise(S, Q, n_img, radius=r, patch_radius=f)
    b = gref.denoise_guided(S, Q, Z, Z, n_img, radius=r, patch_radius=f)
    c = gref.denoise_guided(S, Q, None, None, n_img, radius=r, patch_radius=f)
    assert a.tobytes() == b.tobytes() == c.tobytes()
    assert np.isnan(a).any() and np.isfinite(a).any()


@pytest.mark.parametrize("seed", [1, 2])
def test_step_edge_below_the_noise_is_kept(seed):
    """Measured with the prototype for seeds 1..6: ratio 0.33 - 0.41; the bar is the issue's 0.6."""
    S, Q, F, G, n, truth = gref.step_edge_frame(seed)
    un = denoise_ref.denoise(S, Q, n, radius=10, patch_radius=3, k=0.45, alpha=1.0)
    gd = gref.denoise_guided(S, Q, F, G, n, radius=10, patch_radius=3, k=0.45, alpha=1.0, k_f=0.6, tau=1e-3)
    ru, rg = gref.band_rmse(un, truth), gref.band_rmse(gd, truth)
    print("step edge seed %d: band RMSE unguided %.4f guided %.4f ratio %.3f" % (seed, ru, rg, rg / ru))
    assert rg <= 0.6 * ru


def test_hits_never_mix_with_misses_and_a_nan_feature_falls_back_to_colour():
    S, Q, F, G, n, u = gref.hit_miss_frame()
    un = denoise_ref.denoise(S, Q, n)
    gd = gref.denoise_guided(S, Q, F, G, n)
    assert gd.tobytes() == u.tobytes()  # weights 1 or 0 times dyadic means
    assert np.abs(un - u).max() > 0.2  # the colour weights alone mix across the step
    F2 = F.copy()
    F2[12, 24, 1] = np.nan
    g2 = gref.denoise_guided(S, Q, F2, G, n)
    assert g2[12, 24].tobytes() == un[12, 24].tobytes()  # colour alone for that pixel
    assert np.isfinite(g2).all()
    assert abs(g2[12, 24, 0] - 0.25) > 0.1


def test_radius_zero_is_the_mean():
    rng = np.random.default_rng(1)
    H, W = 9, 13
    S = rng.uniform(0.0, 2.0, (H, W, 3)) * 16
    Q = S * S / 16 + rng.uniform(0.0, 0.5, (H, W, 3))
    S[2, 3, 1] = np.nan
    n = np.full((H, W), 16)
    n[4, 4], n[5, 5] = 1, 0
    F = rng.uniform(0.0, 3.0, (H, W, 7)) * 16
    G = F * F / 16
    F[1, 1, 0] = np.nan
    with np.errstate(all="ignore"):
        mean = S / n[..., None].astype(np.float64)
    for f in (0, 2):
        out = gref.denoise_guided(S, Q, F, G, n, radius=0, patch_radius=f)
        assert out.tobytes() == mean.tobytes()


# ---------------------------------------------------------------- the boundary
def test_new_entry_points_are_exported_and_declared(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    for name in NEW:
        assert name in exported and name in lib.SIGNATURES and name + "(" in header
        assert name in open(os.path.join(ROOT, "integration", "gpu.rs")).read()
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "#define RMD_FEATURE_CHANNELS 7u" in header and abi.RMD_FEATURE_CHANNELS == 7
    assert "#define RMD_ABI_VERSION 6u" in header  # additions within ABI 6
    assert ("rmd_status rmd_denoise_guided(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, const double *feat_dev, "
            "const double *feat_sq_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, "
            "uint32_t n_rects, uint32_t radius, uint32_t patch_radius, double k, double alpha, double k_f, double tau, double *out_dev);") in header


def _last_error(L):
    return (L.rmd_last_error(None) or b"").decode()


def _rects(*rs):
    arr = (abi.TileRect * max(1, len(rs)))()
    for i, (l, t, w, h) in enumerate(rs):
        arr[i].left, arr[i].top, arr[i].width, arr[i].height = l, t, w, h
    return arr


def test_denoise_guided_argument_rules_without_a_device(product_lib):
    L = product_lib
    W, H = 8, 8
    span, fspan = W * H * 3 * 8, W * H * 7 * 8
    base = 0x100000
    s, q, o = C.c_void_p(base), C.c_void_p(base + span), C.c_void_p(base + 2 * span)
    fe, ge = C.c_void_p(base + 3 * span), C.c_void_p(base + 3 * span + fspan)
    full = _rects((0, 0, 8, 8))
    counts = (C.c_uint32 * 2)(4, 4)

    def call(S=s, Q=q, F=fe, G=ge, rects=full, n_rects=1, r=10, f=3, k=0.45, alpha=1.0, kf=0.6, tau=1e-3, out=o):
        return L.rmd_denoise_guided(None, S, Q, F, G, W, H, rects, counts, n_rects, r, f, k, alpha, kf, tau, out)

    def refused(word, **kw):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert word in _last_error(L), (kw, _last_error(L))

    refused("both", F=None)
    refused("both", G=None)
    refused("alias", G=fe)
    refused("alias", G=C.c_void_p(base + 3 * span + 8))
    refused("alias", out=C.c_void_p(base + 3 * span + fspan - 8), Q=C.c_void_p(base + 8 * span))  # out_dev inside the feature range
    refused("alias", Q=s)
    refused("radius", r=13)
    refused("k must", k=0.0)
    for bad in (0.0, -0.6, float("nan"), float("inf")):
        refused("k_f", kf=bad)
        refused("tau", tau=bad)
    refused("outside", rects=_rects((0, 0, 9, 8)))
    refused("overlap", rects=_rects((0, 0, 4, 4), (3, 3, 2, 2)), n_rects=2)
    for kw in ({}, dict(F=None, G=None), dict(F=None, G=None, kf=float("nan"), tau=-1.0), dict(kf=1e-300, tau=1e-300)):  # k_f, tau unread without features
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert _last_error(L) == "null context", (kw, _last_error(L))


def test_render_features_argument_rules_without_a_device(product_lib):
    L = product_lib
    cam = scenes.camera(8, 8).pod()
    st = Settings(scenes.camera(8, 8), 4).pod()
    scene = C.c_void_p(0x200000)  # never looked at: every refusal below comes before the context is
    fe, ge = C.c_void_p(0x100000), C.c_void_p(0x100000 + 8 * 8 * 7 * 8)
    full = _rects((0, 0, 8, 8))

    def call(sc=scene, c=C.byref(cam), s=C.byref(st), rects=full, n=1, F=fe, G=ge, fn=L.rmd_render_features):
        return fn(None, sc, c, s, rects, n, F, G)

    def refused(word, **kw):
        for fn in (L.rmd_render_features, L.rmd_render_features_async):
            assert call(fn=fn, **kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
            assert word in _last_error(L), (kw, _last_error(L))

    refused("null", sc=None)
    refused("null", c=None)
    refused("null", s=None)
    refused("null", F=None)
    refused("null", rects=None)
    refused("alias", G=fe)
    refused("alias", G=C.c_void_p(0x100000 + 8))
    refused("outside", rects=_rects((4, 4, 4, 5)))
    refused("overlap", rects=_rects((0, 0, 8, 8), (0, 0, 8, 8)), n=2)
    for kw in ({}, dict(G=None), dict(rects=None, n=0), dict(rects=_rects((0, 0, 4, 8), (4, 0, 4, 8)), n=2)):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert _last_error(L) == "null context", (kw, _last_error(L))
    assert L.rmd_feature_buffer_alloc(None, 8, 8, C.byref(C.c_void_p())) == abi.RMD_ERR_INVALID_ARGUMENT


def test_settings_feature_defaults_and_rules():
    cam = scenes.camera(64, 64)
    st = Settings(cam, 16)
    assert st.denoise_features is False and st.denoise_feature_k > 0 and st.denoise_feature_tau > 0
    Settings(cam, 16, denoise=True, denoise_features=True, denoise_feature_k=2.0, denoise_feature_tau=1e-6)
    for bad in (dict(denoise_feature_k=0.0), dict(denoise_feature_k=float("nan")), dict(denoise_feature_k=float("inf")), dict(denoise_feature_k=-1.0),
                dict(denoise_feature_tau=0.0), dict(denoise_feature_tau=float("nan")), dict(denoise_feature_tau=float("inf"))):
        with pytest.raises(ValueError):
            Settings(cam, 16, denoise=True, denoise_features=True, **bad)
    with pytest.raises(ValueError):
        Settings(cam, 16, denoise=False, denoise_features=True)  # denoise_features needs denoise


def test_render_tiled_and_await_recheck_feature_settings():
    from raymond_amd import render

    st = Settings(scenes.camera(64, 64), 16, denoise=True, denoise_features=True)
    st.denoise_feature_tau = 0.0
    with pytest.raises(ValueError):
        render.render_tiled(scenes.reflective_spheres(), st)  # refused before a context is created
    st.denoise_feature_tau = 1e-3
    with pytest.raises(ValueError, match="scene"):
        render.TaskHandle(st, [], 0).await_()  # a handle without the scene cannot render features
