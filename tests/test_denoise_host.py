"""rmd_denoise: the parts that need no GPU.

The entry point is exported and declared as the header states it, every argument rule holds before a device is touched, both host mirrors
(Python Settings, raymond_cli) refuse bad denoise settings and the CLI fails loudly without a GPU, and the numpy restatement
(tests/denoise_ref.py) keeps the two exact properties of the definition.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref
from raymond_amd import abi, lib, scenes
from raymond_amd.scene import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")


def test_denoise_is_exported_and_declared(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "rmd_denoise" in set(re.findall(r" T (\w+)", out))
    assert "rmd_denoise" in lib.SIGNATURES
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    assert ("rmd_status rmd_denoise(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height, "
            "const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects, uint32_t radius, uint32_t patch_radius, "
            "double k, double alpha, double *out_dev);") in header
    assert "#define RMD_ABI_VERSION 6u" in header  # an addition within ABI 6
    assert "rmd_denoise" in open(os.path.join(ROOT, "integration", "gpu.rs")).read()
    assert "rmd_denoise" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _last_error(L):
    return (L.rmd_last_error(None) or b"").decode()


def _rects(*rs):
    arr = (abi.TileRect * max(1, len(rs)))()
    for i, (l, t, w, h) in enumerate(rs):
        arr[i].left, arr[i].top, arr[i].width, arr[i].height = l, t, w, h
    return arr


def test_denoise_argument_rules_without_a_device(product_lib):
    """Every bad argument is RMD_ERR_INVALID_ARGUMENT with its own message before the context is looked at; good ones reach 'null context'."""
    L = product_lib
    W, H = 8, 8
    span = W * H * 3 * 8
    s, q, o = C.c_void_p(0x100000), C.c_void_p(0x100000 + span), C.c_void_p(0x100000 + 2 * span)
    full = _rects((0, 0, 8, 8))
    counts = (C.c_uint32 * 2)(4, 4)

    def call(S=s, Q=q, w=W, h=H, rects=full, cnt=counts, n_rects=1, r=10, f=3, k=0.45, alpha=1.0, out=o):
        return L.rmd_denoise(None, S, Q, w, h, rects, cnt, n_rects, r, f, k, alpha, out)

    def refused(word, **kw):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert word in _last_error(L), (kw, _last_error(L))

    refused("bad argument", S=None)
    refused("bad argument", Q=None)
    refused("bad argument", out=None)
    refused("bad argument", w=0)
    refused("bad argument", h=0)
    refused("bad argument", rects=None)
    refused("bad argument", cnt=None)
    refused("alias", Q=s)
    refused("alias", out=s)
    refused("alias", out=q)
    refused("alias", out=C.c_void_p(0x100000 + 2 * span - 8))  # overlapping ranges alias too
    refused("alias", Q=C.c_void_p(0x100000 + 8))
    refused("radius", r=13)
    refused("radius", r=2**32 - 1)
    refused("patch_radius", f=5)
    for k in (0.0, -0.45, float("nan"), float("inf")):
        refused("k must", k=k)
    for a in (-1e-300, -1.0, float("nan"), float("inf")):
        refused("alpha", alpha=a)
    refused("outside", rects=_rects((0, 0, 9, 8)))
    refused("outside", rects=_rects((4, 4, 4, 5)))
    refused("outside", rects=_rects((0, 0, 4, 4), (8, 0, 1, 1)), n_rects=2)
    refused("overlap", rects=_rects((0, 0, 4, 4), (3, 3, 2, 2)), n_rects=2)
    refused("overlap", rects=_rects((0, 0, 8, 8), (0, 0, 8, 8)), n_rects=2)
    # the limits themselves, empty rects and rects that only touch are good arguments: they get as far as the context
    for kw in ({}, dict(r=12, f=4), dict(r=0, f=0), dict(alpha=0.0), dict(k=1e-300), dict(rects=None, cnt=None, n_rects=0),
               dict(rects=_rects((0, 0, 4, 8), (4, 0, 4, 8)), n_rects=2), dict(rects=_rects((0, 0, 0, 8), (0, 0, 8, 8)), n_rects=2)):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert _last_error(L) == "null context", (kw, _last_error(L))


def test_settings_denoise_defaults_and_rules():
    cam = scenes.camera(64, 64)
    st = Settings(cam, 16)
    assert st.denoise is False
    assert (st.denoise_radius, st.denoise_patch, st.denoise_k, st.denoise_alpha) == (10, 3, 0.45, 1.0)
    Settings(cam, 16, denoise=True, denoise_radius=12, denoise_patch=4, denoise_k=2.0, denoise_alpha=0.0)  # the limits are accepted
    Settings(cam, 16, denoise=True, denoise_radius=0, denoise_patch=0)
    for bad in (dict(denoise_radius=13), dict(denoise_radius=-1), dict(denoise_radius=2.5), dict(denoise_patch=5), dict(denoise_patch=-1),
                dict(denoise_k=0.0), dict(denoise_k=-1.0), dict(denoise_k=float("nan")), dict(denoise_k=float("inf")),
                dict(denoise_alpha=-0.5), dict(denoise_alpha=float("nan")), dict(denoise_alpha=float("inf"))):
        with pytest.raises(ValueError):
            Settings(cam, 16, denoise=True, **bad)


def test_render_tiled_rechecks_denoise_settings():
    from raymond_amd import render

    st = Settings(scenes.camera(64, 64), 16, denoise=True)
    st.denoise_patch = 9
    with pytest.raises(ValueError):
        render.render_tiled(scenes.reflective_spheres(), st)  # refused before a context is created


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


def test_cli_refuses_bad_denoise_settings(cli, tmp_path):
    """render_tiled (C++) throws raymond::Error before it starts a worker: no device is needed to see it."""
    for extra in (["--denoise", "1", "--denoise-radius", "13"], ["--denoise", "1", "--denoise-patch", "5"], ["--denoise", "1", "--denoise-k", "0"],
                  ["--denoise", "1", "--denoise-alpha", "-1"], ["--denoise", "1", "--denoise-k", "nan"]):
        r = subprocess.run([cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm"), *extra], capture_output=True, text=True)
        assert r.returncode == 1, (extra, r.stderr)
        assert "denoise" in r.stderr


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK), reason="a GPU is present")
def test_cli_denoise_without_a_gpu_fails_loudly(cli, tmp_path):
    r = subprocess.run([cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm"), "--denoise", "1"], capture_output=True, text=True)
    assert r.returncode != 0
    assert r.stderr.strip()
    assert not (tmp_path / "x.ppm").exists()


# ---------------------------------------------------------------- the restatement's own properties
def _frame(rng, H, W, n):
    S = rng.uniform(0.0, 2.0, (H, W, 3)) * n
    Q = S * S / n + rng.uniform(0.0, 0.5, (H, W, 3))
    return S, Q


def test_reference_radius_zero_is_the_mean():
    rng = np.random.default_rng(1)
    S, Q = _frame(rng, 9, 13, 16)
    S[2, 3, 1] = np.nan
    n = np.full((9, 13), 16)
    n[4, 4], n[5, 5] = 1, 0
    for f in (0, 2, 4):
        out = denoise_ref.denoise(S, Q, n, radius=0, patch_radius=f)
        with np.errstate(all="ignore"):
            mean = S / n[..., None].astype(np.float64)
        assert np.array_equal(out, mean, equal_nan=True)


def test_reference_zero_variance_dyadic_frame_is_unchanged():
    rng = np.random.default_rng(2)
    H, W, n = 11, 17, 8
    u = rng.integers(0, 8, (H, W, 3)) * 0.25  # dyadic means, neighbours equal or at least 0.25 apart
    S = u * n
    Q = S * u  # Q - S*u = 0: zero variance
    for r, f in ((1, 0), (3, 1), (10, 3)):
        out = denoise_ref.denoise(S, Q, np.full((H, W), n), radius=r, patch_radius=f)
        assert np.array_equal(out, u)
