"""rmd_denoise_dual and rmd_tile_error_dual: the parts that need no GPU.

The entry points are exported and declared as the header states them, every argument rule holds before a device is touched, the Python
Settings and raymond_cli refuse the bad combinations, and the numpy restatement (tests/denoise_dual_ref.py) agrees with a per-pixel-loop
reading of the definition and keeps the definition's exact identities.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_dual_ref
import denoise_ref
from raymond_amd import abi, lib, scenes
from raymond_amd.scene import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")


def test_dual_entry_points_are_exported_and_declared(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    assert {"rmd_denoise_dual", "rmd_tile_error_dual"} <= exported
    assert "rmd_denoise_dual" in lib.SIGNATURES and "rmd_tile_error_dual" in lib.SIGNATURES
    assert len(lib.SIGNATURES["rmd_denoise_dual"][1]) == 17 and len(lib.SIGNATURES["rmd_tile_error_dual"][1]) == 7
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    assert ("rmd_status rmd_denoise_dual(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev, "
            "const double *accum_sq_b_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_counts_a, "
            "const uint32_t *rect_counts_b, uint32_t n_rects, uint32_t radius, uint32_t patch_radius, double k, double alpha, double *out_dev, "
            "double *err_dev);") in header
    assert ("rmd_status rmd_tile_error_dual(rmd_context *ctx, const double *err_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects, "
            "uint32_t n_rects, double *out_err_host);") in header
    assert "#define RMD_ABI_VERSION 6u" in header  # additions within ABI 6
    for doc in ("integration/gpu.rs", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "rmd_denoise_dual" in text and "rmd_tile_error_dual" in text, doc


def _last_error(L):
    return (L.rmd_last_error(None) or b"").decode()


def _rects(*rs):
    arr = (abi.TileRect * max(1, len(rs)))()
    for i, (l, t, w, h) in enumerate(rs):
        arr[i].left, arr[i].top, arr[i].width, arr[i].height = l, t, w, h
    return arr


def test_denoise_dual_argument_rules_without_a_device(product_lib):
    """Every bad argument is RMD_ERR_INVALID_ARGUMENT with its own message before the context is looked at; good ones reach 'null context'."""
    L = product_lib
    W, H = 8, 8
    span = W * H * 3 * 8
    base = 0x100000
    sa, qa, sb, qb, o = (C.c_void_p(base + i * span) for i in range(5))
    e = C.c_void_p(base + 5 * span)
    full = _rects((0, 0, 8, 8))
    counts = (C.c_uint32 * 2)(4, 4)

    def call(SA=sa, QA=qa, SB=sb, QB=qb, w=W, h=H, rects=full, ca=counts, cb=counts, n_rects=1, r=10, f=3, k=0.45, alpha=1.0, out=o, err=e):
        return L.rmd_denoise_dual(None, SA, QA, SB, QB, w, h, rects, ca, cb, n_rects, r, f, k, alpha, out, err)

    def refused(word, **kw):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert word in _last_error(L), (kw, _last_error(L))

    for name in ("SA", "QA", "SB", "QB", "out", "rects", "ca", "cb"):
        refused("bad argument", **{name: None})
    refused("bad argument", w=0)
    refused("bad argument", h=0)
    # no two of the six ranges overlap
    names = ["SA", "QA", "SB", "QB", "out", "err"]
    ptrs = [sa, qa, sb, qb, o, e]
    for i in range(6):
        for j in range(6):
            if i != j:
                refused("alias", **{names[i]: ptrs[j]})
    refused("alias", err=C.c_void_p(base + 5 * span - 8))  # err_dev's first double inside out_dev's range
    refused("alias", err=C.c_void_p(base - W * H * 8 + 8))  # err_dev's last double inside accum_a_dev's range
    refused("alias", QB=C.c_void_p(base + 8))
    refused("radius", r=13)
    refused("radius", r=2**32 - 1)
    refused("patch_radius", f=5)
    for k in (0.0, -0.45, float("nan"), float("inf")):
        refused("k must", k=k)
    for a in (-1e-300, -1.0, float("nan"), float("inf")):
        refused("alpha", alpha=a)
    refused("outside", rects=_rects((0, 0, 9, 8)))
    refused("outside", rects=_rects((0, 0, 4, 4), (8, 0, 1, 1)), n_rects=2)
    refused("overlap", rects=_rects((0, 0, 4, 4), (3, 3, 2, 2)), n_rects=2)
    # good arguments get as far as the context: the limits, no error image, err_dev directly behind a range, empty rect lists
    for kw in ({}, dict(r=12, f=4), dict(r=0, f=0), dict(alpha=0.0), dict(err=None), dict(err=C.c_void_p(base - W * H * 8)),
               dict(rects=None, ca=None, cb=None, n_rects=0), dict(rects=_rects((0, 0, 4, 8), (4, 0, 4, 8)), n_rects=2)):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert _last_error(L) == "null context", (kw, _last_error(L))


def test_tile_error_dual_argument_rules_without_a_device(product_lib):
    L = product_lib
    err, out = C.c_void_p(0x100000), (C.c_double * 2)()
    full = _rects((0, 0, 8, 8))

    def call(e=err, w=8, h=8, rects=full, n_rects=1, o=out):
        return L.rmd_tile_error_dual(None, e, w, h, rects, n_rects, o)

    for kw, word in ((dict(e=None), "bad argument"), (dict(w=0), "bad argument"), (dict(h=0), "bad argument"), (dict(rects=None), "bad argument"),
                     (dict(o=None), "bad argument"), (dict(rects=_rects((1, 0, 8, 8))), "outside"), (dict(rects=_rects((0, 7, 1, 2))), "outside")):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert word in _last_error(L), (kw, _last_error(L))
    for kw in ({}, dict(rects=None, o=None, n_rects=0), dict(rects=_rects((8, 8, 0, 0)))):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert _last_error(L) == "null context", (kw, _last_error(L))


def test_settings_dual_defaults_and_rules():
    cam = scenes.camera(64, 64)
    st = Settings(cam, 16)
    assert (st.denoise_dual, st.adaptive_denoised_threshold, st.adaptive_min_samples) == (False, 0.0, 32)
    Settings(cam, 64, denoise=True, denoise_dual=True, samples_per_iteration=8)
    Settings(cam, 64, denoise=True, denoise_dual=True, samples_per_iteration=8, adaptive_denoised_threshold=0.01, adaptive_min_samples=16)
    for bad in (dict(denoise_dual=True, samples_per_iteration=8),  # needs denoise
                dict(denoise=True, denoise_dual=True),  # needs samples_per_iteration > 0
                dict(denoise=True, denoise_dual=True, samples_per_iteration=8, denoise_features=True),
                dict(denoise=True, samples_per_iteration=8, adaptive_denoised_threshold=0.01),  # needs denoise_dual
                dict(denoise=True, denoise_dual=True, samples_per_iteration=8, adaptive_denoised_threshold=0.01, adaptive_threshold=0.1),
                dict(denoise=True, denoise_dual=True, samples_per_iteration=8, adaptive_denoised_threshold=-1.0),
                dict(denoise=True, denoise_dual=True, samples_per_iteration=8, adaptive_denoised_threshold=float("nan")),
                dict(adaptive_min_samples=-1), dict(adaptive_min_samples=2.5)):
        with pytest.raises(ValueError):
            Settings(cam, 64, **bad)
    with pytest.raises(ValueError, match="denoise_features"):  # the message says which combination is refused
        Settings(cam, 64, denoise=True, denoise_dual=True, samples_per_iteration=8, denoise_features=True)


def test_render_tiled_refuses_several_devices_with_denoise_dual():
    from raymond_amd import render

    st = Settings(scenes.camera(64, 64), 16, denoise=True, denoise_dual=True, samples_per_iteration=4)
    with pytest.raises(ValueError, match="one device"):
        render.render_tiled(scenes.reflective_spheres(), st, devices=(0, 1))  # refused before a context is created


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


def test_cli_refuses_bad_dual_settings(cli, tmp_path):
    """render_tiled (C++) throws raymond::Error before it starts a worker: no device is needed to see it."""
    for extra, word in ((["--denoise-dual", "1", "--spi", "4"], "denoise"),  # needs --denoise 1
                        (["--denoise", "1", "--denoise-dual", "1"], "samples_per_iteration"),
                        (["--denoise", "1", "--denoise-dual", "1", "--spi", "4", "--denoise-features", "1"], "denoise_features"),
                        (["--denoise", "1", "--spi", "4", "--adaptive-denoised", "0.01"], "denoise_dual"),
                        (["--denoise", "1", "--denoise-dual", "1", "--spi", "4", "--adaptive-denoised", "0.01", "--adaptive", "0.1"], "exclusive"),
                        (["--denoise", "1", "--denoise-dual", "1", "--spi", "4", "--adaptive-denoised", "-1"], "adaptive_denoised_threshold"),
                        (["--denoise", "1", "--denoise-dual", "1", "--spi", "4", "--gpus", "2"], "one device")):
        r = subprocess.run([cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm"), *extra], capture_output=True, text=True)
        assert r.returncode == 1, (extra, r.stderr)
        assert word in r.stderr, (extra, r.stderr)


# ---------------------------------------------------------------- the restatement's own properties
def _half(rng, H, W, n):
    """Sums and sums of squares of a noisy smooth image at n (H, W) samples per pixel."""
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([0.5 + 0.4 * np.sin(x / 3.0), 0.3 + 0.2 * np.cos(y / 2.0), 0.2 + 0.1 * ((x + y) % 5)], axis=-1)
    nd = np.maximum(n, 1).astype(np.float64)[..., None]
    mean = base + rng.normal(0.0, 0.3, (H, W, 3)) / np.sqrt(nd)
    S = mean * n[..., None]
    Q = S * mean + rng.uniform(0.0, 0.1, (H, W, 3)) * np.maximum(n[..., None] - 1.0, 0.0)
    return S, Q


def _two_halves(seed, H, W):
    rng = np.random.default_rng(seed)
    n_a, n_b = rng.integers(2, 20, (H, W)), rng.integers(2, 20, (H, W))
    n_a[1, 1], n_b[2, 3], n_a[0, 2], n_b[0, 2] = 1, 0, 0, 0  # pixels that are valid in one half only, and in neither
    S_a, Q_a = _half(rng, H, W, n_a)
    S_b, Q_b = _half(rng, H, W, n_b)
    S_a[3, 1, 2], Q_b[4, 4, 0] = np.nan, np.inf
    return S_a, Q_a, S_b, Q_b, n_a, n_b


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("r,f,k,alpha", [(0, 0, 0.45, 1.0), (1, 0, 0.45, 1.0), (2, 1, 0.3, 0.5), (3, 2, 1.0, 0.0)])
def test_restatement_agrees_with_the_per_pixel_reading(r, f, k, alpha):
    """The vectorised restatement against Python loops over pixels, neighbours and patch offsets.  The two take the same operations in the same
    order; numpy's exp of an array and of a scalar may differ in the last bit, hence 4 ulp on a weighted mean."""
    H, W = 7, 9
    halves = _two_halves(11, H, W)
    out, err = denoise_dual_ref.denoise_dual(*halves, radius=r, patch_radius=f, k=k, alpha=alpha)
    out_n, err_n = denoise_dual_ref.denoise_dual_naive(*halves, radius=r, patch_radius=f, k=k, alpha=alpha)
    assert np.array_equal(np.isnan(out), np.isnan(out_n)) and np.array_equal(np.isnan(err), np.isnan(err_n))
    assert np.isnan(err).sum() == 5  # the five pixels that are not dual-valid
    fin = np.isfinite(out_n)
    assert np.all(np.abs(out[fin] - out_n[fin]) <= 4 * np.spacing(np.abs(out_n[fin])))
    fin = np.isfinite(err_n)
    assert np.allclose(err[fin], err_n[fin], rtol=1e-9, atol=1e-30)  # (err is a difference of nearly equal values: judged against the values' ulp)


def test_restatement_radius_zero_is_the_closed_form():
    S_a, Q_a, S_b, Q_b, n_a, n_b = _two_halves(12, 9, 13)
    na, nb = n_a.astype(np.float64)[..., None], n_b.astype(np.float64)[..., None]
    _, _, ok_a = denoise_ref.mean_and_variance(S_a, Q_a, n_a)
    _, _, ok_b = denoise_ref.mean_and_variance(S_b, Q_b, n_b)
    dual = ok_a & ok_b
    with np.errstate(all="ignore"):
        u_a, u_b = S_a / na, S_b / nb
        out_x = np.where(dual[..., None], (na * u_a + nb * u_b) / (na + nb), (S_a + S_b) / (na + nb))
        h = (u_a - u_b) / 2.0
        err_x = np.where(dual, (h[..., 0] * h[..., 0] + h[..., 1] * h[..., 1] + h[..., 2] * h[..., 2]) / 3.0, np.nan)
    for f in (0, 2, 4):
        out, err = denoise_dual_ref.denoise_dual(S_a, Q_a, S_b, Q_b, n_a, n_b, radius=0, patch_radius=f)
        assert out.tobytes() == out_x.tobytes() and err.tobytes() == err_x.tobytes()


@pytest.mark.parametrize("n", [2, 8, 16, 64])
def test_restatement_equal_halves_give_rmd_denoise_and_no_error(n):
    """A == B: f_A == f_B, so err == 0 and out = (n f + n f) / (2 n) = f, exact for the power-of-two counts taken here (n f, its double and the
    division by 2 n are then exact)."""
    rng = np.random.default_rng(13)
    H, W = 12, 15
    n_img = np.full((H, W), n)
    n_img[5, 5] = 1  # a pixel that is not valid in either half
    S, Q = _half(rng, H, W, n_img)
    for r, f in ((1, 0), (3, 1), (5, 2)):
        out, err = denoise_dual_ref.denoise_dual(S, Q, S, Q, n_img, n_img, radius=r, patch_radius=f)
        single = denoise_ref.denoise(S, Q, n_img, radius=r, patch_radius=f)
        assert out.tobytes() == single.tobytes()
        assert np.isnan(err[5, 5]) and np.all(np.delete(err.reshape(-1), 5 * W + 5) == 0.0)


def test_restatement_equal_halves_at_other_counts_are_one_rounding_away():
    """At a count that is not a power of two, n f is rounded and (n f + n f) / (2 n) may miss f by that rounding: the operation order the
    definition states gives this, and the header says so.  err is 0 all the same."""
    rng = np.random.default_rng(14)
    H, W, n = 12, 15, 12
    n_img = np.full((H, W), n)
    S, Q = _half(rng, H, W, n_img)
    out, err = denoise_dual_ref.denoise_dual(S, Q, S, Q, n_img, n_img, radius=3, patch_radius=1)
    single = denoise_ref.denoise(S, Q, n_img, radius=3, patch_radius=1)
    assert np.all(err == 0.0)
    assert np.all(np.abs(out - single) <= np.spacing(np.abs(single)))


def test_restatement_swapping_the_halves():
    S_a, Q_a, S_b, Q_b, n_a, n_b = _two_halves(15, 10, 11)
    out, err = denoise_dual_ref.denoise_dual(S_a, Q_a, S_b, Q_b, n_a, n_b, radius=3, patch_radius=1)
    out_s, err_s = denoise_dual_ref.denoise_dual(S_b, Q_b, S_a, Q_a, n_b, n_a, radius=3, patch_radius=1)
    assert err.tobytes() == err_s.tobytes()  # ((a - b) / 2)^2 == ((b - a) / 2)^2
    # with n_A == n_B the sum of the two products commutes: the same out
    rng = np.random.default_rng(16)
    n = np.full((10, 11), 8)
    n[2, 2] = 1
    A, B = _half(rng, 10, 11, n), _half(rng, 10, 11, n)
    out, err = denoise_dual_ref.denoise_dual(*A, *B, n, n, radius=3, patch_radius=1)
    out_s, err_s = denoise_dual_ref.denoise_dual(*B, *A, n, n, radius=3, patch_radius=1)
    assert out.tobytes() == out_s.tobytes() and err.tobytes() == err_s.tobytes()


def test_restatement_tile_error():
    err = np.arange(48, dtype=np.float64).reshape(6, 8)
    err[4, 6] = np.nan
    rects = [(0, 0, 4, 4), (4, 4, 4, 2), (0, 4, 0, 2), (7, 0, 1, 1)]
    got = denoise_dual_ref.tile_error_dual(err, rects)
    assert got[0] == np.sqrt(err[0:4, 0:4].sum() / 16.0) and got[1] == np.inf and got[2] == 0.0 and got[3] == np.sqrt(7.0)
