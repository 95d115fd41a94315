#!/usr/bin/env python3
"""How much rmd_denoise brings a preview frame towards the converged one (one GPU):

    python tools/denoise_quality.py [--out profiles/r08_denoise/denoise_quality.json] [--ref-spp 2048]
    python tools/denoise_quality.py --guided [--out profiles/r09_features/denoise_quality.json]
    python tools/denoise_quality.py --slope [--out profiles/r20_slope/slope_quality.json]

For ReflectiveSpheres and the small GoldDragon stand-in (n = 24) at 256x144: frames of 16, 64 and 256 spp with moments are denoised, and the
RMSE of the noisy and of the denoised frame against a --ref-spp frame of another seed is reported with its ratio, first at the default
parameters (r 10, f 3, k 0.45, alpha 1), then over a small sweep of k, alpha, r and f at 16 and 64 spp.  The converged-frame check denoises a
--ref-spp frame and compares its distance to a second --ref-spp frame (a third seed) with their own distance.

--guided: rmd_denoise_guided against rmd_denoise on the same sums instead.  At 16 and 64 spp, k_f in {0.3, 0.6, 1.0} x tau in {1e-4, 1e-3, 1e-2}
x k in {0.45, 0.6}: whole-frame RMSE, and RMSE over the pixels within 2 px of a change of first-hit object (found from the converged albedo and
depth means), guided and unguided at the SAME k; and the converged-frame check of the guided filter for every (k_f, tau) at k = 0.45.

--slope: rmd_denoise_guided_slope.  At 16 and 64 spp, slope in {0, 1, 2, 3, 5, 8} x k in {0.45, 0.6} x (k_f, tau) in {(1.0, 1e-2), (0.6, 1e-3)}: whole-frame
and edge-pixel RMSE, beside the unguided filter's at the same k; and the converged-frame check at the values the header recommends (k 0.45, k_f 1.0,
tau 1e-2) for every slope.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raymond_amd import render, scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

DEFAULT = dict(radius=10, patch_radius=3, k=0.45, alpha=1.0)
SWEEP = [dict(DEFAULT, k=k) for k in (0.3, 0.6, 0.8)] + [dict(DEFAULT, alpha=a) for a in (0.5, 2.0)] + \
        [dict(DEFAULT, radius=r, patch_radius=f) for r, f in ((5, 2), (12, 4), (10, 1))]


def moments(ctx, ds, W, H, spp, seed):
    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=seed)
    fb, fb_sq = render.Framebuffer(ctx, W, H), render.Framebuffer(ctx, W, H)
    try:
        render.render_tiles(ctx, ds, st.camera_settings, st, generate_tiles(W, H, (32, 32)), fb, 0, spp, framebuffer_sq=fb_sq)
        return fb.download(), fb_sq.download()
    finally:
        fb.close(), fb_sq.close()


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def feature_sums(ctx, ds, W, H, spp, seed):
    st = Settings(scenes.camera(W, H), sample_count=spp, bounce_limit=5, seed=seed)
    fb, fb_sq = render.FeatureBuffer(ctx, W, H), render.FeatureBuffer(ctx, W, H)
    try:
        render.render_features(ctx, ds, st.camera_settings, st, generate_tiles(W, H, (32, 32)), fb, 0, spp, features_sq=fb_sq)
        return fb.download(), fb_sq.download()
    finally:
        fb.close(), fb_sq.close()


def edge_mask(f):
    """Pixels within 2 px of a change of first-hit object: where the converged albedo or relative depth of 4-neighbours differs."""
    key = np.concatenate([f[..., 3:6], f[..., 6:7] / np.maximum(f[..., 6:7].max(), 1e-300)], axis=-1)
    e = np.zeros(f.shape[:2], dtype=bool)
    dx = np.abs(key[:, 1:] - key[:, :-1]).max(axis=-1) > 0.02
    dy = np.abs(key[1:] - key[:-1]).max(axis=-1) > 0.02
    e[:, 1:] |= dx
    e[:, :-1] |= dx
    e[1:] |= dy
    e[:-1] |= dy
    out = e.copy()
    for _ in range(2):  # dilate by 2 px
        g = out.copy()
        g[1:] |= out[:-1]
        g[:-1] |= out[1:]
        g[:, 1:] |= out[:, :-1]
        g[:, :-1] |= out[:, 1:]
        out = g
    return out


def guided_main(a):
    W, H = 256, 144
    out = {"width": W, "height": H, "ref_spp": a.ref_spp, "unguided_default": DEFAULT, "scenes": {}}
    rect = [(0, 0, W, H)]
    with render.Context(0) as ctx:
        for name, scene in (("reflective_spheres", scenes.reflective_spheres()), ("gold_dragon_standin_n24", scenes.gold_dragon_standin(n=24))):
            ds = render.DeviceScene(ctx, scene)
            try:
                S_ref, Q_ref = moments(ctx, ds, W, H, a.ref_spp, seed=0x1234567)
                S_ref2, _ = moments(ctx, ds, W, H, a.ref_spp, seed=0x7654321)
                F_ref, G_ref = feature_sums(ctx, ds, W, H, a.ref_spp, 0x1234567)
                ref, ref2 = S_ref / a.ref_spp, S_ref2 / a.ref_spp
                edge = edge_mask(F_ref / a.ref_spp)
                rec = {"edge_pixel_fraction": float(edge.mean()), "sweep": [], "converged": []}
                own = rmse(ref, ref2)
                for kf in (0.3, 0.6, 1.0):
                    for tau in (1e-4, 1e-3, 1e-2):
                        den = render.denoise_guided_arrays(ctx, S_ref, Q_ref, F_ref, G_ref, rect, [a.ref_spp], k_f=kf, tau=tau, **DEFAULT)
                        rec["converged"].append({"k_f": kf, "tau": tau, "ratio": rmse(den, ref2) / own})
                for spp in (16, 64):
                    S, Q = moments(ctx, ds, W, H, spp, seed=scenes.SEED)
                    F, G = feature_sums(ctx, ds, W, H, spp, scenes.SEED)
                    for k in (0.45, 0.6):
                        p = dict(DEFAULT, k=k)
                        un = render.denoise_arrays(ctx, S, Q, rect, [spp], **p)
                        row = {"spp": spp, "k": k, "unguided": {"rmse": rmse(un, ref), "rmse_edge": rmse(un[edge], ref[edge])}, "guided": []}
                        for kf in (0.3, 0.6, 1.0):
                            for tau in (1e-4, 1e-3, 1e-2):
                                gd = render.denoise_guided_arrays(ctx, S, Q, F, G, rect, [spp], k_f=kf, tau=tau, **p)
                                row["guided"].append({"k_f": kf, "tau": tau, "rmse": rmse(gd, ref), "rmse_edge": rmse(gd[edge], ref[edge])})
                        rec["sweep"].append(row)
                        print(name, json.dumps(row), flush=True)
                out["scenes"][name] = rec
                print(name, json.dumps(rec["converged"]), flush=True)
            finally:
                ds.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


SLOPES = (0.0, 1.0, 2.0, 3.0, 5.0, 8.0)
SLOPE_GUIDES = ((1.0, 1e-2), (0.6, 1e-3))


def slope_main(a):
    W, H = 256, 144
    out = {"width": W, "height": H, "ref_spp": a.ref_spp, "unguided_default": DEFAULT, "slopes": SLOPES, "scenes": {}}
    rect = [(0, 0, W, H)]
    with render.Context(0) as ctx:
        for name, scene in (("reflective_spheres", scenes.reflective_spheres()), ("gold_dragon_standin_n24", scenes.gold_dragon_standin(n=24))):
            ds = render.DeviceScene(ctx, scene)
            try:
                S_ref, Q_ref = moments(ctx, ds, W, H, a.ref_spp, seed=0x1234567)
                S_ref2, _ = moments(ctx, ds, W, H, a.ref_spp, seed=0x7654321)
                F_ref, G_ref = feature_sums(ctx, ds, W, H, a.ref_spp, 0x1234567)
                ref, ref2 = S_ref / a.ref_spp, S_ref2 / a.ref_spp
                edge = edge_mask(F_ref / a.ref_spp)
                rec = {"edge_pixel_fraction": float(edge.mean()), "sweep": [], "converged": []}
                own = rmse(ref, ref2)
                for slope in SLOPES:  # at the recommended k, k_f and tau
                    den = render.denoise_guided_arrays(ctx, S_ref, Q_ref, F_ref, G_ref, rect, [a.ref_spp], k_f=1.0, tau=1e-2, slope=slope, **DEFAULT)
                    rec["converged"].append({"slope": slope, "ratio": rmse(den, ref2) / own})
                for spp in (16, 64):
                    S, Q = moments(ctx, ds, W, H, spp, seed=scenes.SEED)
                    F, G = feature_sums(ctx, ds, W, H, spp, scenes.SEED)
                    for k in (0.45, 0.6):
                        p = dict(DEFAULT, k=k)
                        un = render.denoise_arrays(ctx, S, Q, rect, [spp], **p)
                        for kf, tau in SLOPE_GUIDES:
                            row = {"spp": spp, "k": k, "k_f": kf, "tau": tau, "unguided": {"rmse": rmse(un, ref), "rmse_edge": rmse(un[edge], ref[edge])}, "slopes": []}
                            for slope in SLOPES:
                                gd = render.denoise_guided_arrays(ctx, S, Q, F, G, rect, [spp], k_f=kf, tau=tau, slope=slope, **p)
                                row["slopes"].append({"slope": slope, "rmse": rmse(gd, ref), "rmse_edge": rmse(gd[edge], ref[edge])})
                            rec["sweep"].append(row)
                            print(name, json.dumps(row), flush=True)
                out["scenes"][name] = rec
                print(name, json.dumps(rec["converged"]), flush=True)
            finally:
                ds.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--guided", action="store_true")
    ap.add_argument("--slope", action="store_true")
    a = ap.parse_args()
    if a.guided:
        return guided_main(a)
    if a.slope:
        return slope_main(a)
    W, H = 256, 144
    out = {"width": W, "height": H, "ref_spp": a.ref_spp, "default": DEFAULT, "scenes": {}}
    with render.Context(0) as ctx:
        for name, scene in (("reflective_spheres", scenes.reflective_spheres()), ("gold_dragon_standin_n24", scenes.gold_dragon_standin(n=24))):
            ds = render.DeviceScene(ctx, scene)
            try:
                S_ref, Q_ref = moments(ctx, ds, W, H, a.ref_spp, seed=0x1234567)
                S_ref2, _ = moments(ctx, ds, W, H, a.ref_spp, seed=0x7654321)
                ref, ref2 = S_ref / a.ref_spp, S_ref2 / a.ref_spp
                rec = {"levels": [], "sweep": []}
                for spp in (16, 64, 256):
                    S, Q = moments(ctx, ds, W, H, spp, seed=scenes.SEED)
                    noisy = rmse(S / spp, ref)
                    den = rmse(render.denoise_arrays(ctx, S, Q, [(0, 0, W, H)], [spp], **DEFAULT), ref)
                    rec["levels"].append({"spp": spp, "rmse_noisy": noisy, "rmse_denoised": den, "ratio": den / noisy})
                    if spp in (16, 64):
                        for p in SWEEP:
                            d = rmse(render.denoise_arrays(ctx, S, Q, [(0, 0, W, H)], [spp], **p), ref)
                            rec["sweep"].append({"spp": spp, "params": p, "rmse_denoised": d, "ratio": d / noisy})
                own = rmse(ref, ref2)
                den = rmse(render.denoise_arrays(ctx, S_ref, Q_ref, [(0, 0, W, H)], [a.ref_spp], **DEFAULT), ref2)
                rec["converged"] = {"rmse_between_refs": own, "rmse_denoised_to_second": den, "ratio": den / own}
                out["scenes"][name] = rec
                print(name, json.dumps(rec["levels"]), json.dumps(rec["converged"]), flush=True)
            finally:
                ds.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
