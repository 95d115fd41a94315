"""rmd_denoise_atrous_dual: the parts that need no GPU.

The entry point is exported and declared as the header states it, every argument rule holds before a device is touched and carries its own text,
both host mirrors (Python Settings, raymond_cli) refuse bad settings, and the numpy restatement (tests/denoise_atrous_dual_ref.py) agrees with its
pixel-by-pixel reading and keeps the definition's exact properties.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_atrous_dual_ref as adref
import denoise_atrous_ref as aref
import denoise_guided_ref as gref
import denoise_ref
import test_denoise_dual_host as tdh
from raymond_amd import abi, lib, scenes
from raymond_amd.scene import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")


# ---------------------------------------------------------------- the boundary
def test_entry_point_is_exported_and_declared(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "rmd_denoise_atrous_dual" in set(re.findall(r" T (\w+)", out))
    assert "rmd_denoise_atrous_dual" in lib.SIGNATURES and len(lib.SIGNATURES["rmd_denoise_atrous_dual"][1]) == 21
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    assert ("rmd_status rmd_denoise_atrous_dual(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev, "
            "const double *accum_sq_b_dev, const double *feat_dev, const double *feat_sq_dev, uint32_t width, uint32_t height, "
            "const rmd_tile_rect *rects, const uint32_t *rect_counts_a, const uint32_t *rect_counts_b, const uint32_t *rect_counts_f, uint32_t n_rects, "
            "uint32_t levels, double k, double alpha, double k_f, double tau, double *out_dev, double *err_dev);") in header
    assert "#define RMD_ABI_VERSION 6u" in header  # an addition within ABI 6
    fault_list = header[header.index("RMD_ERR_DEVICE_FAULT = 8") : header.index("rmd_denoise_atrous) */")]
    assert "rmd_denoise_atrous_dual," in fault_list  # among the calls that report an earlier fault
    assert "rmd_denoise_atrous_dual" in open(os.path.join(ROOT, "integration", "gpu.rs")).read()
    assert "rmd_denoise_atrous_dual" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _last_error(L):
    return (L.rmd_last_error(None) or b"").decode()


def _rects(*rs):
    arr = (abi.TileRect * max(1, len(rs)))()
    for i, (l, t, w, h) in enumerate(rs):
        arr[i].left, arr[i].top, arr[i].width, arr[i].height = l, t, w, h
    return arr


def test_argument_rules_without_a_device(product_lib):
    L = product_lib
    W, H = 8, 8
    span, fspan = W * H * 3 * 8, W * H * 7 * 8
    base = 0x100000
    sa, qa, sb, qb, o = (C.c_void_p(base + i * span) for i in range(5))
    e = C.c_void_p(base + 5 * span)
    fe, ge = C.c_void_p(base + 6 * span), C.c_void_p(base + 6 * span + fspan)
    full = _rects((0, 0, 8, 8))
    counts = (C.c_uint32 * 2)(4, 4)

    def call(SA=sa, QA=qa, SB=sb, QB=qb, F=fe, G=ge, w=W, h=H, rects=full, ca=counts, cb=counts, cf=counts, n_rects=1, levels=5, k=3.0, alpha=1.0, kf=1.0,
             tau=1e-2, out=o, err=e):
        return L.rmd_denoise_atrous_dual(None, SA, QA, SB, QB, F, G, w, h, rects, ca, cb, cf, n_rects, levels, k, alpha, kf, tau, out, err)

    def refused(word, **kw):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        msg = _last_error(L)
        assert msg.startswith("rmd_denoise_atrous_dual: ") and word in msg, (kw, msg)

    for kw in (dict(SA=None), dict(QA=None), dict(SB=None), dict(QB=None), dict(out=None), dict(w=0), dict(h=0), dict(rects=None), dict(ca=None), dict(cb=None)):
        refused("bad argument", **kw)
    refused("both", F=None)
    refused("both", G=None)
    refused("rect_counts_f is NULL", cf=None)
    alias = "the sum buffers, out_dev and err_dev must not alias"
    refused(alias, QA=sa)
    refused(alias, SB=C.c_void_p(base + span - 8))  # partial overlap
    refused(alias, out=C.c_void_p(base + 8))
    refused(alias, err=C.c_void_p(base + 4 * span + 8))  # err_dev inside out_dev
    refused(alias, err=C.c_void_p(base + 5 * span - span // 3 + 8))  # err_dev's W*H doubles reach into out_dev
    falias = "feat_dev and feat_sq_dev must not alias each other, the sum buffers, out_dev or err_dev"
    refused(falias, G=fe)
    refused(falias, G=C.c_void_p(base + 6 * span + 8))
    refused(falias, F=C.c_void_p(base + 5 * span + 8))  # inside err_dev
    refused(falias, out=C.c_void_p(base + 6 * span + fspan - 8), err=None)
    refused("levels must be <= 8", levels=9)
    refused("levels must be <= 8", levels=2**32 - 1)
    for bad in (0.0, -3.0, float("nan"), float("inf")):
        refused("k must be finite and > 0", k=bad)
        refused("k_f must be finite and > 0", kf=bad)
        refused("tau must be finite and > 0", tau=bad)
    for bad in (-1.0, float("nan"), float("inf")):
        refused("alpha must be finite and >= 0", alpha=bad)
    refused("outside", rects=_rects((0, 0, 9, 8)))
    refused("outside", rects=_rects((4, 4, 4, 5)))
    refused("overlap", rects=_rects((0, 0, 4, 4), (3, 3, 2, 2)), n_rects=2)
    # the good edge cases reach the context: levels 0 and 8, alpha 0, no rects, no error image, NULL features whose counts, k_f and tau are not read
    for kw in ({}, dict(levels=0), dict(levels=8), dict(alpha=0.0), dict(rects=None, ca=None, cb=None, cf=None, n_rects=0), dict(err=None),
               dict(F=None, G=None), dict(F=None, G=None, cf=None, kf=float("nan"), tau=-1.0), dict(rects=_rects((0, 0, 4, 8), (4, 0, 4, 8)), n_rects=2)):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert _last_error(L) == "null context", (kw, _last_error(L))


# ---------------------------------------------------------------- the host mirrors
def test_settings_defaults_and_rules():
    cam = scenes.camera(64, 64)
    assert Settings(cam, 16).denoise_dual_atrous is False
    dual = dict(denoise=True, denoise_dual=True, samples_per_iteration=4)
    st = Settings(cam, 16, denoise_dual_atrous=True, **dual)
    assert st.denoise_dual_atrous is True and st.denoise_atrous is False
    Settings(cam, 16, denoise_dual_atrous=True, denoise_dual_features=True, adaptive_denoised_threshold=0.01, denoise_atrous_levels=0, **dual)
    with pytest.raises(ValueError, match="denoise_dual_atrous needs denoise_dual"):
        Settings(cam, 16, denoise_dual_atrous=True)
    with pytest.raises(ValueError, match="denoise_dual_atrous needs denoise_dual"):
        Settings(cam, 16, denoise=True, denoise_dual_atrous=True)
    with pytest.raises(ValueError, match="denoise_dual_atrous cannot be combined with denoise_dual_select"):
        Settings(cam, 16, denoise_dual_atrous=True, denoise_dual_select=True, **dual)
    with pytest.raises(ValueError, match="denoise_atrous_levels"):
        Settings(cam, 16, denoise_dual_atrous=True, denoise_atrous_levels=9, **dual)
    with pytest.raises(ValueError, match="rmd_denoise_atrous has no dual form"):  # the single filter's own setting is still refused beside denoise_dual
        Settings(cam, 16, denoise_atrous=True, denoise_dual_atrous=True, **dual)


def test_render_tiled_and_await_recheck_the_settings():
    from raymond_amd import render

    st = Settings(scenes.camera(64, 64), 16, denoise=True, denoise_dual=True, samples_per_iteration=4, denoise_dual_atrous=True)
    st.denoise_dual_select = True
    with pytest.raises(ValueError, match="denoise_dual_select"):
        render.render_tiled(scenes.reflective_spheres(), st)  # refused before a context is created
    with pytest.raises(ValueError, match="denoise_dual_select"):
        render.TaskHandle(st, [], 0).await_()
    st.denoise_dual_select = False
    st.denoise_dual_features = True
    with pytest.raises(ValueError, match="scene"):
        render.TaskHandle(st, [], 0).await_()  # a handle without the scene cannot render features


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


def test_cli_refuses_bad_dual_atrous_settings(cli, tmp_path):
    """render_tiled (C++) throws raymond::Error before it starts a worker: no device is needed to see it."""
    dual = ["--denoise", "1", "--denoise-dual", "1", "--spi", "4"]
    for extra, word in ((["--denoise-dual-atrous", "1"], "denoise_dual_atrous needs denoise_dual"),
                        (["--denoise", "1", "--denoise-dual-atrous", "1"], "denoise_dual_atrous needs denoise_dual"),
                        (dual + ["--denoise-dual-atrous", "1", "--denoise-dual-select", "1"], "denoise_dual_atrous cannot be combined with denoise_dual_select"),
                        (dual + ["--denoise-dual-atrous", "1", "--denoise-atrous-levels", "9"], "denoise_atrous_levels"),
                        (dual + ["--denoise-dual-atrous", "1", "--denoise-atrous", "1"], "denoise_atrous cannot be combined with denoise_dual")):
        r = subprocess.run([cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm"), *extra], capture_output=True, text=True)
        assert r.returncode == 1, (extra, r.stderr)
        assert word in r.stderr, (extra, r.stderr)


# ---------------------------------------------------------------- the restatement's own properties
def _features(rng, H, W, n_f):
    """Feature sums and sums of squares at the (H, W) counts n_f: a plane that tilts, two albedos, and a NaN and an inf among them."""
    y, x = np.mgrid[0:H, 0:W]
    f = np.zeros((H, W, 7))
    f[..., 0], f[..., 2] = 0.1 * np.sin(x / 2.0), 1.0
    f[..., 3:6] = np.where((x + y)[..., None] % 4 < 2, 0.8, 0.3)
    f[..., 6] = 2.0 + 0.05 * y
    nd = n_f.astype(np.float64)[..., None]
    F = f * nd
    G = F * f + rng.uniform(0.0, 0.01, (H, W, 7)) * np.maximum(nd - 1.0, 0.0)
    if H * W > 1:
        F[H - 1, 0, 3], G[0, W - 1, 6] = np.nan, np.inf
    return F, G


def _frame(W, H, seed):
    """test_denoise_dual_host._two_halves' inputs (pixels valid in one half only and in neither, NaN / inf in S and Q) with features at their own count."""
    if W * H == 1:
        rng = np.random.default_rng(seed)
        n_a, n_b = np.full((1, 1), 5), np.full((1, 1), 7)
        halves = (*tdh._half(rng, 1, 1, n_a), *tdh._half(rng, 1, 1, n_b), n_a, n_b)
    else:
        halves = tdh._two_halves(seed, H, W)
    rng = np.random.default_rng(seed + 1)
    n_f = halves[4] + halves[5]
    if W * H > 1:
        n_f[H - 1, W - 1], n_f[H - 2, 1] = 1, 3  # a pixel without feature variance, and a count that is not n_A + n_B
    return halves, _features(rng, H, W, n_f), n_f


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (13, 9)])
def test_the_two_readings_agree_bit_for_bit(W, H):
    halves, (F, G), n_f = _frame(W, H, 100 * W + H)
    for levels in (0, 1, 3, 8):
        for guide in ({}, dict(F=F, G=G, n_f=n_f)):
            a = adref.atrous_dual(*halves, levels=levels, **guide)
            b = adref.atrous_dual_by_pixel(*halves, levels=levels, **guide)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (levels, bool(guide))
    if W * H > 1:  # the frame exercised something: the five pixels that are not dual-valid, and features that change the result
        assert np.isnan(a[1]).sum() == 5 and np.isfinite(a[0]).any()
        un, gd = adref.atrous_dual(*halves, levels=3), adref.atrous_dual(*halves, levels=3, F=F, G=G, n_f=n_f)
        assert not np.array_equal(un[0], gd[0], equal_nan=True) and not np.array_equal(un[1], gd[1], equal_nan=True)


def test_levels_zero_is_the_closed_form():
    (S_a, Q_a, S_b, Q_b, n_a, n_b), (F, G), n_f = _frame(13, 9, 12)
    na, nb = n_a.astype(np.float64)[..., None], n_b.astype(np.float64)[..., None]
    _, _, ok_a = denoise_ref.mean_and_variance(S_a, Q_a, n_a)
    _, _, ok_b = denoise_ref.mean_and_variance(S_b, Q_b, n_b)
    dual = ok_a & ok_b
    with np.errstate(all="ignore"):
        u_a, u_b = S_a / na, S_b / nb
        out_x = np.where(dual[..., None], (na * u_a + nb * u_b) / (na + nb), (S_a + S_b) / (na + nb))
        h = (u_a - u_b) / 2.0
        err_x = np.where(dual, (h[..., 0] * h[..., 0] + h[..., 1] * h[..., 1] + h[..., 2] * h[..., 2]) / 3.0, np.nan)
    for guide in ({}, dict(F=F, G=G, n_f=n_f)):
        out, err = adref.atrous_dual(S_a, Q_a, S_b, Q_b, n_a, n_b, levels=0, **guide)
        assert out.tobytes() == out_x.tobytes() and err.tobytes() == err_x.tobytes()


@pytest.mark.parametrize("n", [2, 8, 16, 64])
def test_equal_halves_give_rmd_denoise_atrous_and_no_error(n):
    """A == B: both passes take the single filter's operations, so f_A == f_B == rmd_denoise_atrous of either half, err == 0, and
    out = (n f + n f) / (2 n) = f exactly at the power-of-two counts taken here."""
    rng = np.random.default_rng(13)
    H, W = 12, 15
    n_img = np.full((H, W), n)
    n_img[5, 5] = 1  # a pixel that is not valid in either half
    S, Q = tdh._half(rng, H, W, n_img)
    F, G = _features(rng, H, W, n_img)
    for levels in (1, 3, 5):
        for guide, single_guide in (({}, {}), (dict(F=F, G=G, n_f=n_img), dict(F=F, G=G))):
            out, err = adref.atrous_dual(S, Q, S, Q, n_img, n_img, levels=levels, **guide)
            single = aref.atrous(S, Q, n_img, levels=levels, **single_guide)
            keep = np.ones((H, W), dtype=bool)
            keep[5, 5] = False  # (there the dual call gives the MERGED mean 2 S / 2 n and NaN)
            assert out[keep].tobytes() == single[keep].tobytes(), (levels, bool(guide))
            assert np.isnan(err[5, 5]) and np.all(err[keep] == 0.0)
    assert not np.array_equal(aref.atrous(S, Q, n_img, levels=3)[keep], aref.atrous(S, Q, n_img, levels=3, F=F, G=G)[keep])


@pytest.mark.parametrize("levels", [1, 3, 5])
def test_zero_features_are_the_unguided_bytes(levels):
    halves, _, n_f = _frame(37, 23, 37023)
    n_f = np.maximum(n_f, 2)
    Z = np.zeros((23, 37, 7))
    a = adref.atrous_dual(*halves, levels=levels)
    b = adref.atrous_dual(*halves, levels=levels, F=Z, G=Z, n_f=n_f)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert np.isnan(a[1]).any() and np.isfinite(a[1]).any()


def test_hit_miss_frame_in_two_equal_halves_is_exact_guided_and_not_unguided():
    S, Q, F, G, n, u = gref.hit_miss_frame()
    for levels in (1, 2, 5, 8):
        out, err = adref.atrous_dual(S, Q, S, Q, n, n, levels=levels, F=F, G=G, n_f=n)
        assert out.tobytes() == u.tobytes() and np.all(err == 0.0), levels  # weights h or 0 times dyadic means; n = 8 is a power of two
        un, _ = adref.atrous_dual(S, Q, S, Q, n, n, levels=levels)
        assert un.tobytes() != u.tobytes(), levels
    assert np.abs(un - u).max() > 0.1  # the colour weights alone mix across the step
