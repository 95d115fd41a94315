"""rmd_denoise_dual_region: the parts that need no GPU.

The entry point is exported and declared as the header states it (an addition within ABI 6), and every argument rule — rmd_denoise_dual's own, and
the three of the region — holds before a device is touched.
"""
import ctypes as C
import os
import re
import subprocess

from raymond_amd import abi, lib
from test_denoise_dual_host import _last_error, _rects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_region_entry_point_is_exported_and_declared(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    assert {"rmd_denoise_dual_region", "rmd_denoise_dual", "rmd_tile_error_dual"} <= exported
    assert "rmd_denoise_dual_region" in lib.SIGNATURES
    assert len(lib.SIGNATURES["rmd_denoise_dual_region"][1]) == 19
    assert len(lib.SIGNATURES["rmd_denoise_dual"][1]) == 17  # the whole-frame call keeps its signature
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    assert ("rmd_status rmd_denoise_dual_region(rmd_context *ctx, const double *accum_a_dev, const double *accum_sq_a_dev, const double *accum_b_dev, "
            "const double *accum_sq_b_dev, uint32_t width, uint32_t height, const rmd_tile_rect *rects, const uint32_t *rect_counts_a, "
            "const uint32_t *rect_counts_b, uint32_t n_rects, const rmd_tile_rect *region, uint32_t n_region, uint32_t radius, uint32_t patch_radius, "
            "double k, double alpha, double *out_dev, double *err_dev);") in header
    assert "#define RMD_ABI_VERSION 6u" in header  # an addition within ABI 6
    for doc in ("integration/gpu.rs", "INTEGRATION.md"):
        assert "rmd_denoise_dual_region" in open(os.path.join(ROOT, doc)).read(), doc


def test_denoise_dual_region_argument_rules_without_a_device(product_lib):
    """Every bad argument is RMD_ERR_INVALID_ARGUMENT with its own message before the context is looked at; good ones reach 'null context'."""
    L = product_lib
    W, H = 8, 8
    span = W * H * 3 * 8
    base = 0x100000
    sa, qa, sb, qb, o = (C.c_void_p(base + i * span) for i in range(5))
    e = C.c_void_p(base + 5 * span)
    full = _rects((0, 0, 8, 8))
    counts = (C.c_uint32 * 2)(4, 4)
    some = _rects((1, 2, 3, 4))

    def call(SA=sa, QA=qa, SB=sb, QB=qb, w=W, h=H, rects=full, ca=counts, cb=counts, n_rects=1, region=some, n_region=1, r=10, f=3, k=0.45, alpha=1.0, out=o,
             err=e):
        return L.rmd_denoise_dual_region(None, SA, QA, SB, QB, w, h, rects, ca, cb, n_rects, region, n_region, r, f, k, alpha, out, err)

    def refused(word, **kw):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        message = _last_error(L)
        assert word in message and message.startswith("rmd_denoise_dual_region: "), (kw, message)
        return message

    # rmd_denoise_dual's rules
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
    refused("alias", QB=C.c_void_p(base + 8))
    refused("radius", r=13)
    refused("radius", r=2**32 - 1)
    refused("patch_radius", f=5)
    for k in (0.0, -0.45, float("nan"), float("inf")):
        refused("k must", k=k)
    for a in (-1e-300, -1.0, float("nan"), float("inf")):
        refused("alpha", alpha=a)
    frame_outside = refused("outside", rects=_rects((0, 0, 9, 8)))
    refused("outside", rects=_rects((0, 0, 4, 4), (8, 0, 1, 1)), n_rects=2)
    frame_overlap = refused("overlap", rects=_rects((0, 0, 4, 4), (3, 3, 2, 2)), n_rects=2)
    # the region's own three, each with a text of its own
    null_region = refused("region", region=None)
    region_outside = refused("outside", region=_rects((0, 0, 9, 8)))
    refused("outside", region=_rects((0, 0, 4, 4), (8, 0, 1, 1)), n_region=2)
    refused("outside", region=_rects((2**32 - 1, 0, 2, 1)))  # left + width wraps in 32 bits
    region_overlap = refused("overlap", region=_rects((0, 0, 4, 4), (3, 3, 2, 2)), n_region=2)
    assert "region" in region_outside and "region" in region_overlap
    assert len({null_region, region_outside, region_overlap, frame_outside, frame_overlap}) == 5
    # good arguments get as far as the context: the limits, no error image, an empty region (NULL or not), one that is not cut as the rects are, the
    # whole frame, rects without pixels, and no rects at all
    for kw in ({}, dict(r=12, f=4), dict(r=0, f=0), dict(alpha=0.0), dict(err=None), dict(region=None, n_region=0), dict(n_region=0),
               dict(region=_rects((0, 0, 8, 8))), dict(region=_rects((0, 0, 1, 1), (7, 7, 1, 1), (3, 1, 4, 5)), n_region=3),
               dict(region=_rects((8, 8, 0, 0), (0, 0, 0, 8), (0, 0, 8, 8)), n_region=3), dict(rects=None, ca=None, cb=None, n_rects=0),
               dict(rects=_rects((0, 0, 4, 8), (4, 0, 4, 8)), n_rects=2, region=_rects((3, 0, 2, 8)))):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert _last_error(L) == "null context", (kw, _last_error(L))
