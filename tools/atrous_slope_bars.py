"""The CPU figures behind the quality test of tests/test_gpu_denoise_atrous_slope.py.

    python tools/atrous_slope_bars.py [--out profiles/r21_atrous_slope/atrous_slope_bars.json] [--threads 0] [--scenes spheres mesh] [--slopes 2 3 5]

No GPU: the oracle's per-sample frames, tests/first_hit_ref.first_hit_sums for the features and the numpy restatement
(tests/denoise_atrous_slope_ref.py).  ReflectiveSpheres and the mesh stand-in at 256 x 144, 16 spp of scenes.SEED, 5 bounces, against 2,048 spp of
scenes.SEED + 1; the shipped levels, k, alpha, k_f and tau.  Per scene: RMSE of the unfiltered mean, of the unguided filter, of the guided filter
(slope 0) and of each slope, and each slope's ratio to the guided filter.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import denoise_atrous_slope_ref as asref  # noqa: E402
import first_hit_ref  # noqa: E402
import oracle_lib  # noqa: E402
from raymond_amd import scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

SPP, REF_SPP = 16, 2048


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_atrous_slope", "atrous_slope_bars.json"))
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--scenes", nargs="*", default=["spheres", "mesh"])
    ap.add_argument("--slopes", type=float, nargs="*", default=[2.0, 3.0, 5.0])
    ap.add_argument("--size", type=int, nargs=2, default=[256, 144])
    ap.add_argument("--ref-spp", type=int, default=REF_SPP)
    a = ap.parse_args()
    W, H = a.size
    cam = scenes.camera(W, H)
    tiles = generate_tiles(W, H, (32, 32))
    st = Settings(cam, SPP)  # the shipped defaults
    kw = dict(levels=st.denoise_atrous_levels, k=st.denoise_atrous_k, alpha=st.denoise_alpha)
    guide = dict(k_f=st.denoise_feature_k, tau=st.denoise_feature_tau)
    result = {"width": W, "height": H, "spp": SPP, "reference_spp": a.ref_spp, **kw, **guide, "scenes": {}}
    for which in a.scenes:
        sc = scenes.reflective_spheres() if which == "spheres" else scenes.gold_dragon_standin(n=24)
        osc = oracle_lib.OracleScene(sc, fast=True)
        ref = osc.render_tiles(cam, Settings(cam, sample_count=a.ref_spp, bounce_limit=5, seed=scenes.SEED + 1), tiles, threads=a.threads) / float(a.ref_spp)
        S, Q = np.zeros((H, W, 3)), np.zeros((H, W, 3))
        for s in range(SPP):  # one oracle pass per sample, so that each sample's square is known
            smp = osc.render_tiles(cam, Settings(cam, sample_count=1, bounce_limit=5, seed=scenes.SEED), [(0, 0, W, H)], sample_begin=s, sample_count=1, threads=a.threads)
            S, Q = S + smp, Q + smp * smp
        osc.close()
        F, G, _ = first_hit_ref.first_hit_sums(sc, cam, scenes.SEED, SPP)
        n = np.full((H, W), SPP)
        row = {"rmse_unfiltered": rmse(S / float(SPP), ref), "rmse_unguided": rmse(asref.atrous_slope(S, Q, n, **kw), ref),
               "rmse_guided": rmse(asref.atrous_slope(S, Q, n, F=F, G=G, slope=0.0, **kw, **guide), ref), "slopes": {}}
        for slope in a.slopes:
            r = rmse(asref.atrous_slope(S, Q, n, F=F, G=G, slope=slope, **kw, **guide), ref)
            row["slopes"]["%g" % slope] = {"rmse": r, "ratio_to_guided": r / row["rmse_guided"]}
        result["scenes"][which] = row
        print(which, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
