#!/usr/bin/env python3
"""What the per-pixel choice among dual-buffer filters gains, and how well SURE estimates a filter's error (one GPU):

    python tools/dual_select_quality.py [--out profiles/r13_select/dual_select_quality.json] [--ref-spp 2048]

For ReflectiveSpheres and the small GoldDragon stand-in (n = 24) at 256x144, 5 bounces, against a --ref-spp frame of seed + 1 (whose own noise is part
of every RMSE), at 32 and 64 samples in passes of 8 that alternate between the halves, the features of all the samples, r = 10, f = 3, alpha = 1, both
windows 2.  Every candidate of CANDIDATES alone (rmd_denoise_dual_select with one candidate: that filter's frame and its per-pixel SURE) and every
selection of SELECTIONS: the RMSE; sqrt(mean sure) and sqrt(mean err) over the true RMSE; over the 32 x 32 tiles, Spearman's rank correlation of the
tile's mean SURE (and of rmd_tile_error_dual) with the tile's true RMS error, and the number of tiles whose mean SURE is negative; for a selection the
share of pixels each candidate wins.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

from dual_quality import BOUNCES, H, SPI, W, rmse, spearman, tile_rms  # noqa: E402  (tools/ is this script's directory)

CANDIDATES = {
    "unguided_k0.45": dict(k=0.45),
    "unguided_k1.0": dict(k=1.0),
    "guided_k0.45": dict(k=0.45, guided=True, k_f=1.0, tau=1e-2),
    "guided_k0.6": dict(k=0.6, guided=True, k_f=1.0, tau=1e-2),
    "guided_k1.0": dict(k=1.0, guided=True, k_f=1.0, tau=1e-2),
    "guided_k0.45_kf0.6_tau1e-3": dict(k=0.45, guided=True, k_f=0.6, tau=1e-3),
}
SELECTIONS = {
    "select_default": ["unguided_k0.45", "guided_k1.0"],  # Settings.denoise_dual_select
    "select_k_only": ["unguided_k0.45", "unguided_k1.0"],
    "select_four": ["unguided_k0.45", "guided_k1.0", "guided_k0.6", "unguided_k1.0"],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ref-spp", type=int, default=2048)
    a = ap.parse_args()
    tiles, whole = generate_tiles(W, H, (32, 32)), [(0, 0, W, H)]
    out = {"width": W, "height": H, "bounces": BOUNCES, "samples_per_iteration": SPI, "ref_spp": a.ref_spp, "radius": 10, "patch_radius": 3, "alpha": 1.0,
           "sure_window": 2, "select_window": 2, "candidates": CANDIDATES, "selections": SELECTIONS, "scenes": {}}
    with render.Context(0) as ctx:
        for name, scene in (("reflective_spheres", scenes.reflective_spheres()), ("gold_dragon_standin_n24", scenes.gold_dragon_standin(n=24))):
            opened = [render.DeviceScene(ctx, scene)]
            try:
                ds = opened[0]
                fbs = [render.Framebuffer(ctx, W, H) for _ in range(5)]
                feat = [render.FeatureBuffer(ctx, W, H) for _ in range(2)]
                err, sure, win = render.ErrorImage(ctx, W, H), render.ErrorImage(ctx, W, H), render.WinnerImage(ctx, W, H)
                opened += fbs + feat + [err, sure, win]
                st = Settings(scenes.camera(W, H), sample_count=a.ref_spp, bounce_limit=BOUNCES, seed=scenes.SEED + 1)
                render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fbs[4])
                ref = fbs[4].download() / a.ref_spp
                rec = []
                for spp in (32, 64):
                    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=BOUNCES, seed=scenes.SEED)
                    for b in fbs[:4] + feat:
                        b.zero()
                    for j in range(spp // SPI):
                        render.render_tiles(ctx, ds, st.camera_settings, st, tiles, fbs[2 * (j & 1)], j * SPI, SPI, framebuffer_sq=fbs[2 * (j & 1) + 1])
                    render.render_features(ctx, ds, st.camera_settings, st, tiles, feat[0], 0, spp, features_sq=feat[1])
                    row = {"samples": spp, "rmse_noisy": rmse((fbs[0].download() + fbs[2].download()) / float(spp), ref), "filters": {}}
                    for label, names in list((n, [n]) for n in CANDIDATES) + list(SELECTIONS.items()):
                        render.denoise_dual_select(ctx, (fbs[0], fbs[1]), (fbs[2], fbs[3]), whole, [spp // 2], [spp // 2], [CANDIDATES[n] for n in names], fbs[4], err,
                                                   sure, win, radius=10, patch_radius=3, sure_window=2, select_window=2, features=feat[0], features_sq=feat[1],
                                                   counts_f=[spp])
                        frame, e, s, w = fbs[4].download(), err.download(), sure.download(), win.download()
                        true = tile_rms(frame, ref, tiles)
                        tile_sure = np.array([s[t : t + h, l : l + w_].mean() for (l, t, w_, h) in tiles])
                        r = rmse(frame, ref)
                        row["filters"][label] = {
                            "rmse": r, "root_mean_sure_over_rmse": float(np.sqrt(max(s.mean(), 0.0))) / r, "root_mean_err_over_rmse": float(np.sqrt(e.mean())) / r,
                            "tiles_spearman_sure_true": spearman(tile_sure, true), "tiles_spearman_err_true": spearman(render.tile_error_dual(ctx, err, tiles), true),
                            "tiles_with_negative_mean_sure": int((tile_sure < 0.0).sum()), "tiles": len(tiles),
                            "win_share": [float((w == i).mean()) for i in range(len(names))]}
                    f = row["filters"]
                    for sel, names in SELECTIONS.items():
                        f[sel]["rmse_over_best_candidate"] = f[sel]["rmse"] / min(f[n]["rmse"] for n in names)
                        f[sel]["rmse_over_worst_candidate"] = f[sel]["rmse"] / max(f[n]["rmse"] for n in names)
                        f[sel]["rmse_over_best_single_filter"] = f[sel]["rmse"] / min(f[n]["rmse"] for n in CANDIDATES)
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
