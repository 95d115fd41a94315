#!/usr/bin/env python3
"""The bytes every denoise entry point and rmd_tile_error_dual give for one small poisoned frame, as SHA-256 of each output array:

    RAYMOND_HIP_LIB=<a build of the commit to record> python tools/record_denoise_bits.py --recorded-from <that commit> \\
        --out tests/golden/denoise_bits.json

One GPU.  The frame is 70 x 37: a remainder against every tile shape in play (32 and 24 wide by 16 high, 64 by 4, rows of 256 threads), and a level-3 tap
(step 4) still crosses it.  The inputs are integer arithmetic on index arrays — a fixed 64-bit mix, then IEEE multiplications, additions and divisions —, so
they depend on no generator's version and no file; the fixture keeps their SHA-256 too.  Rects: generate_tiles(70, 37, (32, 16)) with one left out
(n = 0), one at count 1 (not valid), the others at counts from 2 upward with counts_a != counts_b; the feature counts are the sums.  One pixel has +inf
in a sum, one a NaN in a sum of squares of half B only, one a NaN in a feature square.  The region forms get two rects that align to no tile and
start from fixed non-zero out and err images, so the pixels they leave alone are hashed too.

tests/test_gpu_denoise_bits.py replays CASES against the library under test and wants every hash equal: the numpy restatements the rest of the suite
compares with hold to 1e-9, which cannot show that a kernel compiled from shared code still gives the same bytes.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import render  # noqa: E402
from raymond_amd.scene import generate_tiles  # noqa: E402

W, H = 70, 37
TILES = generate_tiles(W, H, (32, 16))  # column-major: 3 columns (32, 32, 6 wide) of 3 rows (16, 16, 5 high)
LEFT_OUT, COUNT_ONE = 7, 5  # (64, 16, 6, 16) is in no rect; (32, 32, 32, 5) holds one sample per half
RECTS = [t for i, t in enumerate(TILES) if i != LEFT_OUT]
COUNTS_A = [1 if t == TILES[COUNT_ONE] else 2 + 3 * i for i, t in enumerate(RECTS)]
COUNTS_B = [1 if t == TILES[COUNT_ONE] else 3 + 5 * i for i, t in enumerate(RECTS)]
COUNTS_F = [a + b for a, b in zip(COUNTS_A, COUNTS_B)]
REGION = [(5, 3, 29, 13), (41, 19, 27, 15)]  # across the first two tiles of the top row; across four tiles, the one left out and the one at count 1 among them
INF_SUM, NAN_SQ_B, NAN_FEAT_SQ = (12, 8), (50, 25), (20, 22)  # (x, y): inside the first region rect, inside the second, outside both
NLM = [(0, 0), (3, 1), (12, 4)]  # (radius, patch radius); the last runs the 24-wide tile
GUIDE = dict(k_f=0.6, tau=1e-3)
CANDIDATES = [dict(k=0.45), dict(k=0.9, alpha=0.5), dict(k=0.45, guided=True, **GUIDE)]


def _mix(salt, *shape):
    """[0, 1) doubles with 53 random bits: splitmix64's finalizer over the element index, offset by `salt`."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53).reshape(shape)


def _count_image(counts):
    n = np.zeros((H, W), dtype=np.float64)
    for (x, y, w, h), c in zip(RECTS, counts):
        n[y:y + h, x:x + w] = c
    return n


def _sums(salt, n, mean, channels):
    """Sums and sums of squares of n samples per pixel around `mean`: S = n * (mean + noise), Q = S*S / n + (n - 1) * (a per-sample variance)."""
    n = np.maximum(n, 1.0)[:, :, None]
    S = n * (mean + 0.08 * (_mix(salt, H, W, channels) - 0.5))
    Q = S * S / n + (n - 1.0) * (0.002 + 0.03 * _mix(salt + 1000003, H, W, channels))
    return S, Q


def inputs():
    """{name: array}: the halves' sums SA, QA, SB, QB (H, W, 3), the features' F, G (H, W, 7), and what the region forms' outputs hold before the call."""
    yy, xx = np.mgrid[0:H, 0:W]
    # flat patches with edges between them, a ramp across the frame: both kinds of weight occur
    base = 0.15 + 0.3 * ((xx // 11 + 2 * (yy // 9)) % 3) + 0.002 * xx
    colour = np.stack([base, 0.9 - base * 0.5, 0.3 + 0.4 * ((xx // 17) % 2)], axis=2)
    feat = np.stack([colour[:, :, 0], colour[:, :, 1], colour[:, :, 2], ((xx // 11) % 2) * 1.0, ((yy // 9) % 2) * 1.0, 0.5 + 0.0 * xx, 2.0 + 0.05 * xx + 0.1 * (yy // 9)], axis=2)
    SA, QA = _sums(11, _count_image(COUNTS_A), colour, 3)
    SB, QB = _sums(22, _count_image(COUNTS_B), colour, 3)
    F, G = _sums(33, _count_image(COUNTS_F), feat, 7)
    SA[INF_SUM[1], INF_SUM[0], 1] = np.inf
    QB[NAN_SQ_B[1], NAN_SQ_B[0], 2] = np.nan
    G[NAN_FEAT_SQ[1], NAN_FEAT_SQ[0], 4] = np.nan
    return {"SA": SA, "QA": QA, "SB": SB, "QB": QB, "F": F, "G": G, "out_init": 1.0 + _mix(44, H, W, 3), "err_init": 1.0 + _mix(55, H, W)}


def sha(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


def _single(fn, guided, **params):
    def run(ctx, x):
        feats = (x["F"], x["G"]) if guided else (None, None)
        if fn is render.denoise_arrays:
            return {"out": fn(ctx, x["SA"], x["QA"], RECTS, COUNTS_A, **params)}
        return {"out": fn(ctx, x["SA"], x["QA"], *feats, RECTS, COUNTS_A, **(dict(GUIDE, **params) if guided else params))}
    return run


def _dual(fn, guided, region, **params):
    def run(ctx, x):
        kw = dict(features=x["F"], features_sq=x["G"], counts_f=COUNTS_F, **GUIDE) if guided else {}
        if region:
            kw.update(region=REGION, out_init=x["out_init"], err_init=x["err_init"])
        out, err = fn(ctx, x["SA"], x["QA"], x["SB"], x["QB"], RECTS, COUNTS_A, COUNTS_B, **kw, **params)
        return {"out": out} if err is None else {"out": out, "err": err}
    return run


def _select(ctx, x):
    return render.denoise_dual_select_arrays(ctx, x["SA"], x["QA"], x["SB"], x["QB"], RECTS, COUNTS_A, COUNTS_B, CANDIDATES, features=x["F"], features_sq=x["G"],
                                             counts_f=COUNTS_F, radius=3, patch_radius=1, sure_window=2, select_window=2)


def _tile_error(ctx, x):
    """rmd_tile_error_dual over the error image of rmd_denoise_dual at (3, 1), as this library makes it: over the tiles (the one left out too) and the region's rects."""
    _, err = render.denoise_dual_arrays(ctx, x["SA"], x["QA"], x["SB"], x["QB"], RECTS, COUNTS_A, COUNTS_B, radius=3, patch_radius=1)
    img = render.ErrorImage(ctx, W, H)
    try:
        img.upload(err)
        return {"tile_error": render.tile_error_dual(ctx, img, TILES + REGION).copy()}
    finally:
        img.close()


def _cases():
    c = {}
    for r, f in NLM:
        c["rmd_denoise r=%d f=%d" % (r, f)] = _single(render.denoise_arrays, False, radius=r, patch_radius=f)
    for r, f in NLM[1:]:
        c["rmd_denoise_guided r=%d f=%d" % (r, f)] = _single(render.denoise_guided_arrays, True, radius=r, patch_radius=f)
    for guided in (False, True):
        for levels in (0, 1, 3):
            c["rmd_denoise_atrous levels=%d%s" % (levels, " guided" if guided else "")] = _single(render.denoise_atrous_arrays, guided, levels=levels)
    for region in (False, True):
        for guided in (False, True):
            for r, f in NLM[1:]:
                name = "rmd_denoise_dual%s%s r=%d f=%d" % ("_guided" if guided else "", "_region" if region else "", r, f)
                c[name] = _dual(render.denoise_dual_arrays, guided, region, radius=r, patch_radius=f)
    c["rmd_denoise_dual_select"] = _select
    for region in (False, True):
        for guided in (False, True):
            for levels in (0, 1, 3):
                name = "rmd_denoise_atrous_dual%s levels=%d%s" % ("_region" if region else "", levels, " guided" if guided else "")
                want_err = not (levels == 1 and not guided)  # one of each form without an error image
                c[name + ("" if want_err else " no err")] = _dual(render.denoise_atrous_dual_arrays, guided, region, levels=levels, want_err=want_err)
    c["rmd_tile_error_dual"] = _tile_error
    return c


CASES = _cases()  # {case id: fn(ctx, inputs) -> {output name: array}}, in the fixture's order


def device_name():
    """Device 0's name and architecture string out of hipGetDeviceProperties: the name leads the struct, the architecture is found by its "gfx"."""
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    buf = C.create_string_buffer(16384)  # (hipDeviceProp_t is some 1.5 KB)
    fn = getattr(hip, "hipGetDevicePropertiesR0600", None) or hip.hipGetDeviceProperties
    if fn(buf, 0) != 0:
        return "unknown"
    raw = buf.raw
    arch = raw[raw.find(b"gfx"):].split(b"\0")[0] if b"gfx" in raw else b""
    return (raw[:256].split(b"\0")[0] + b" " + arch).decode(errors="replace").strip() or "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--recorded-from", required=True, help="what RAYMOND_HIP_LIB was built from, for the file's header (a commit, say)")
    a = ap.parse_args()
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    x = inputs()
    doc = {"about": "tools/record_denoise_bits.py; recorded from: %s.  SHA-256 of every input and of every output array's bytes, per case" % a.recorded_from,
           "frame": [W, H], "hipcc": subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.splitlines()[0],
           "inputs": {k: sha(v) for k, v in x.items()}, "cases": {}}
    with render.Context(0) as ctx:
        doc["device"] = device_name()
        for name, fn in CASES.items():
            doc["cases"][name] = {k: sha(v) for k, v in fn(ctx, x).items()}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("%d cases -> %s (%d bytes); %s; %s" % (len(CASES), a.out, os.path.getsize(a.out), doc["hipcc"], doc["device"]))


if __name__ == "__main__":
    main()
