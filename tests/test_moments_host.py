"""Per-pixel second moments and adaptive tile sampling: the parts that need no GPU.

The three ABI 6 entry points are exported and declared in the ctypes table, their argument rules hold before any device is touched, the
version mirrors agree, and both host mirrors (Python Settings, raymond_cli) refuse adaptive settings that render_tiled cannot follow.
"""
import ctypes as C
import os
import re
import subprocess

import pytest

from raymond_amd import abi, lib, scenes
from raymond_amd.scene import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
NEW = ("rmd_render_tiles_moments", "rmd_render_tiles_moments_async", "rmd_tile_error")


def test_moments_entry_points_are_exported_and_declared(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    header = open(os.path.join(ROOT, "include", "raymond_hip.h")).read()
    for name in NEW:
        assert name in exported
        assert name in lib.SIGNATURES
        assert re.search(r"rmd_status %s\(" % name, header)


def test_abi_version_is_6_everywhere(product_lib):
    header = open(os.path.join(ROOT, "include", "raymond_hip.h")).read()
    assert abi.RMD_ABI_VERSION == 6
    assert int(re.search(r"#define RMD_ABI_VERSION (\d+)u", header).group(1)) == 6
    assert product_lib.rmd_abi_version() == 6
    assert "const RMD_ABI_VERSION: u32 = 6;" in open(os.path.join(ROOT, "integration", "gpu.rs")).read()
    assert "RMD_ABI_VERSION (6)" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _last_error(L):
    return (L.rmd_last_error(None) or b"").decode()


def test_moments_argument_rules_without_a_device(product_lib):
    """NULL context, an aliased second buffer and a bad floor come back as RMD_ERR_INVALID_ARGUMENT before a device is needed."""
    L = product_lib
    cam, st = abi.Camera(), abi.Settings()
    cam.backbuffer_width = cam.backbuffer_height = 8
    st.bounce_limit, st.sample_count = 2, 1
    rect = (abi.TileRect * 1)()
    rect[0].width = rect[0].height = 8
    fake_a, fake_b = C.c_void_p(0x1000), C.c_void_p(0x2000)
    for fn in (L.rmd_render_tiles_moments, L.rmd_render_tiles_moments_async):
        # the aliasing rule is checked first: its own message, context or not
        assert fn(None, None, C.byref(cam), C.byref(st), rect, 1, fake_a, fake_a) == abi.RMD_ERR_INVALID_ARGUMENT
        assert "alias" in _last_error(L)
        # a NULL context (with or without the second buffer), as rmd_render_tiles
        assert fn(None, None, C.byref(cam), C.byref(st), rect, 1, fake_a, fake_b) == abi.RMD_ERR_INVALID_ARGUMENT
        assert fn(None, None, C.byref(cam), C.byref(st), rect, 1, fake_a, None) == abi.RMD_ERR_INVALID_ARGUMENT
    out = (C.c_double * 1)()
    te = L.rmd_tile_error
    assert te(None, fake_a, fake_a, 8, 8, 4, 1e-3, rect, 1, out) == abi.RMD_ERR_INVALID_ARGUMENT
    assert "alias" in _last_error(L)
    for floor in (0.0, -1.0, float("nan"), float("inf")):
        assert te(None, fake_a, fake_b, 8, 8, 4, floor, rect, 1, out) == abi.RMD_ERR_INVALID_ARGUMENT
        assert "floor" in _last_error(L)
    assert te(None, None, fake_b, 8, 8, 4, 1e-3, rect, 1, out) == abi.RMD_ERR_INVALID_ARGUMENT
    assert te(None, fake_a, None, 8, 8, 4, 1e-3, rect, 1, out) == abi.RMD_ERR_INVALID_ARGUMENT
    assert te(None, fake_a, fake_b, 8, 8, 4, 1e-3, None, 1, out) == abi.RMD_ERR_INVALID_ARGUMENT
    assert te(None, fake_a, fake_b, 8, 8, 4, 1e-3, rect, 1, None) == abi.RMD_ERR_INVALID_ARGUMENT
    assert te(None, fake_a, fake_b, 8, 8, 4, 1e-3, rect, 1, out) == abi.RMD_ERR_INVALID_ARGUMENT  # NULL context
    assert _last_error(L) == "null context"


def test_settings_adaptive_defaults_and_rules():
    cam = scenes.camera(64, 64)
    st = Settings(cam, 16)
    assert st.adaptive_threshold == 0.0 and st.adaptive_floor == 1e-3
    Settings(cam, 16, samples_per_iteration=4, adaptive_threshold=0.05)  # accepted
    Settings(cam, 16, adaptive_threshold=0.0)  # off: no passes needed
    with pytest.raises(ValueError):
        Settings(cam, 16, samples_per_iteration=4, adaptive_threshold=-0.1)
    with pytest.raises(ValueError):
        Settings(cam, 16, samples_per_iteration=0, adaptive_threshold=0.05)
    with pytest.raises(ValueError):
        Settings(cam, 16, samples_per_iteration=4, adaptive_threshold=0.05, adaptive_floor=0.0)
    with pytest.raises(ValueError):
        Settings(cam, 16, samples_per_iteration=4, adaptive_threshold=float("nan"))


def test_render_tiled_rechecks_settings_changed_after_construction():
    from raymond_amd import render

    st = Settings(scenes.camera(64, 64), 16, samples_per_iteration=4, adaptive_threshold=0.05)
    st.samples_per_iteration = 0
    with pytest.raises(ValueError):
        render.render_tiled(scenes.reflective_spheres(), st)  # refused before a context is created


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


def test_cli_refuses_adaptive_without_spi(cli, tmp_path):
    """render_tiled (C++) throws raymond::Error before it starts a worker: no device is needed to see it."""
    for extra in (["--adaptive", "0.05"], ["--adaptive", "-1", "--spi", "4"], ["--adaptive", "0.05", "--spi", "4", "--adaptive-floor", "0"]):
        r = subprocess.run([cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm"), *extra], capture_output=True, text=True)
        assert r.returncode == 1, (extra, r.stderr)
        assert "adaptive" in r.stderr
