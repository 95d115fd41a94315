#!/usr/bin/env python3
"""What the feature weight changes in the dual-buffer filter's frame and in its error estimate (one GPU):

    python tools/dual_guided_quality.py [--out profiles/r12_dual_guided/dual_guided_quality.json] [--ref-spp 2048]

For ReflectiveSpheres and the small GoldDragon stand-in (n = 24) at 256x144, 5 bounces, 32 x 32 tiles, against a --ref-spp frame of seed + 1
(whose own noise is part of every RMSE), at 8 + 8, 16 + 16, 32 + 32 and 64 + 64 samples in the two halves (A: the first half of the samples, B: the
second), the features of all the samples at the shipped k_f and tau: the RMSE of rmd_denoise_dual and of rmd_denoise_dual_guided on the same
halves, and for each the median over the tiles of rmd_tile_error_dual / the tile's true RMS error, and Spearman's rank correlation of the two.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

from dual_quality import BOUNCES, H, W, rmse, spearman, tile_rms  # noqa: E402  (tools/ is this script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ref-spp", type=int, default=2048)
    a = ap.parse_args()
    tiles = generate_tiles(W, H, (32, 32))
    whole = [(0, 0, W, H)]
    defaults = Settings(scenes.camera(W, H), 16)  # the shipped filter parameters
    params = dict(radius=defaults.denoise_radius, patch_radius=defaults.denoise_patch, k=defaults.denoise_k, alpha=defaults.denoise_alpha)
    out = {"width": W, "height": H, "bounces": BOUNCES, "ref_spp": a.ref_spp, "k_f": defaults.denoise_feature_k, "tau": defaults.denoise_feature_tau, **params,
           "scenes": {}}
    with render.Context(0) as ctx:
        for name, scene in (("reflective_spheres", scenes.reflective_spheres()), ("gold_dragon_standin_n24", scenes.gold_dragon_standin(n=24))):
            opened = [render.DeviceScene(ctx, scene)]
            try:
                ds = opened[0]
                fbs = [render.Framebuffer(ctx, W, H) for _ in range(5)]
                err = render.ErrorImage(ctx, W, H)
                opened += fbs + [err]
                st = Settings(scenes.camera(W, H), sample_count=a.ref_spp, bounce_limit=BOUNCES, seed=scenes.SEED + 1)
                render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fbs[4])
                ref = fbs[4].download() / a.ref_spp
                rec = []
                for half in (8, 16, 32, 64):
                    st = Settings(scenes.camera(W, H), sample_count=2 * half, bounce_limit=BOUNCES, seed=scenes.SEED)
                    feat = [render.FeatureBuffer(ctx, W, H) for _ in range(2)]
                    opened += feat
                    for fb in fbs[:4]:
                        fb.zero()
                    render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fbs[0], 0, half, framebuffer_sq=fbs[1])
                    render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fbs[2], half, half, framebuffer_sq=fbs[3])
                    render.render_features(ctx, ds, st.camera_settings, st, tiles, feat[0], 0, 2 * half, features_sq=feat[1])
                    row = {"samples_per_half": half, "rmse_noisy": rmse((fbs[0].download() + fbs[2].download()) / (2.0 * half), ref)}
                    for label, kw in (("rmd_denoise_dual", {}),
                                      ("rmd_denoise_dual_guided", dict(features=feat[0], features_sq=feat[1], counts_f=[2 * half], k_f=defaults.denoise_feature_k,
                                                                       tau=defaults.denoise_feature_tau))):
                        render.denoise_dual(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), whole, [half], [half], fbs[4], err, **params, **kw)
                        frame, estimate = fbs[4].download(), render.tile_error_dual(ctx, err, tiles)
                        true = tile_rms(frame, ref, tiles)
                        row[label] = {"rmse": rmse(frame, ref), "median_estimate_over_true": float(np.median(estimate / true)),
                                      "spearman_estimate_true": spearman(estimate, true)}
                    row["rmse_guided_over_unguided"] = row["rmd_denoise_dual_guided"]["rmse"] / row["rmd_denoise_dual"]["rmse"]
                    rec.append(row)
                    print(name, json.dumps(row), flush=True)
                out["scenes"][name] = rec
            finally:
                for o in reversed(opened):
                    o.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
