#!/usr/bin/env python3
"""The a-trous filter's quality beside the non-local means filters, at 256x144 (one GPU):

    python tools/atrous_quality.py [--out profiles/r14_atrous/atrous_quality.json]

ReflectiveSpheres and the mesh scene (gold_dragon_standin(n=24)), 5 bounces, 8 / 16 / 32 / 64 spp of the project's seed; RMSE in linear radiance
against 2,048 spp of seed + 1.  rmd_denoise_atrous at k in {2, 3, 4}, levels in {3, 5}, guided (k_f 1.0, tau 1e-2) and unguided, beside the
unfiltered mean, rmd_denoise and rmd_denoise_guided at their defaults on the same sums.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402


def moments(ctx, ds, W, H, spp, seed, features):
    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=seed)
    tiles = generate_tiles(W, H, (32, 32))
    fb, fb_sq = render.Framebuffer(ctx, W, H), render.Framebuffer(ctx, W, H)
    ft, ft_sq = render.FeatureBuffer(ctx, W, H), render.FeatureBuffer(ctx, W, H)
    try:
        render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fb, 0, spp, framebuffer_sq=fb_sq)
        if features:
            render.render_features(ctx, ds, st.camera_settings, st, tiles, ft, 0, spp, features_sq=ft_sq)
        return fb.download(), fb_sq.download(), ft.download(), ft_sq.download()
    finally:
        for b in (fb, fb_sq, ft, ft_sq):
            b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = 256, 144
    rect = [(0, 0, W, H)]
    result = {"width": W, "height": H, "bounces": 5, "reference_spp": 2048, "scenes": {}}
    with render.Context(0) as ctx:
        for name, sc in (("ReflectiveSpheres", scenes.reflective_spheres()), ("mesh", scenes.gold_dragon_standin(n=24))):
            ds = render.DeviceScene(ctx, sc)
            try:
                ref = moments(ctx, ds, W, H, 2048, scenes.SEED + 1, False)[0] / 2048.0
                rmse = lambda img: float(np.sqrt(np.mean((img - ref) ** 2)))  # noqa: E731
                per_spp = {}
                for spp in (8, 16, 32, 64):
                    S, Q, F, G = moments(ctx, ds, W, H, spp, scenes.SEED, True)
                    row = {"unfiltered": rmse(S / float(spp)), "rmd_denoise": rmse(render.denoise_arrays(ctx, S, Q, rect, [spp])),
                           "rmd_denoise_guided": rmse(render.denoise_guided_arrays(ctx, S, Q, F, G, rect, [spp]))}
                    for k in (2.0, 3.0, 4.0):
                        for levels in (3, 5):
                            row["atrous_k%g_l%d_unguided" % (k, levels)] = rmse(render.denoise_atrous_arrays(ctx, S, Q, None, None, rect, [spp], levels=levels, k=k))
                            row["atrous_k%g_l%d_guided" % (k, levels)] = rmse(render.denoise_atrous_arrays(ctx, S, Q, F, G, rect, [spp], levels=levels, k=k))
                    per_spp[str(spp)] = row
                    print(name, spp, json.dumps(row), flush=True)
                result["scenes"][name] = per_spp
            finally:
                ds.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
