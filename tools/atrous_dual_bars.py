"""The two quality bars of tests/test_gpu_denoise_atrous_dual.py, measured on the CPU.

    python tools/atrous_dual_bars.py [--out profiles/r15_atrous_dual/atrous_dual_bars.json] [--threads 0]

No GPU: the oracle's per-sample frames and the numpy restatement (tests/denoise_atrous_dual_ref.py).  ReflectiveSpheres and the mesh stand-in at
256 x 144, 5 bounces: samples [0, 8) of a seed are half A, [8, 16) half B; the converged frame is 2,048 spp of scenes.SEED + 1.  The shipped
defaults (5 levels, k 3.0, alpha 1, unguided).  Over three seeds, per scene:
  (a) RMSE of the dual frame / RMSE of the single filter (denoise_atrous_ref.atrous) on the merged sums
  (b) Spearman's rank correlation over the 32 x 32 tiles between tile_error_dual of err and the tile's true RMS error
and the bars the device test asserts: (a) the largest ratio plus twice the spread, (b) the smallest correlation minus twice the spread, the
spread being largest minus smallest over the three seeds.

    --levels 3 5      also, per seed, the dual frame's RMSE and the rank correlation at each of these level counts (one run of the restatement to the
                      largest of them), under "by_levels" — the comparison DESIGN.md section 19 makes between 3 and 5 levels for the adaptive check.
                      The bars stay those of 5 levels.
    --ref-spp N, --seeds N   a smaller converged frame and fewer seeds than the bars' own 2,048 and 3
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

import denoise_atrous_dual_ref as adref  # noqa: E402
import denoise_atrous_ref as aref  # noqa: E402
import denoise_dual_ref  # noqa: E402
import oracle_lib  # noqa: E402
from raymond_amd import scenes  # noqa: E402
from raymond_amd.scene import Settings, generate_tiles  # noqa: E402

W, H, HALF, REF_SPP = 256, 144, 8, 2048


def spearman(a, b):
    """Spearman's rank correlation: Pearson's on the ranks, ties at their mean rank."""
    def ranks(v):
        v = np.asarray(v, dtype=np.float64)
        order = np.argsort(v, kind="stable")
        r = np.empty(len(v))
        r[order] = np.arange(len(v), dtype=np.float64)
        for x in np.unique(v):
            m = v == x
            r[m] = r[m].mean()
        return r

    ra, rb = ranks(a), ranks(b)
    ra, rb = ra - ra.mean(), rb - rb.mean()
    return float((ra * rb).sum() / np.sqrt((ra * ra).sum() * (rb * rb).sum()))


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def tile_true_rms(img, ref, tiles):
    return [rmse(img[t : t + h, l : l + w], ref[t : t + h, l : l + w]) for (l, t, w, h) in tiles]


def half_sums(osc, cam, seed, begin, threads):
    """S and Q of samples [begin, begin + HALF): one oracle pass per sample, so that each sample's square is known."""
    full = [(0, 0, W, H)]
    S, Q = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    for s in range(begin, begin + HALF):
        st = Settings(cam, sample_count=1, bounce_limit=5, seed=seed)
        smp = osc.render_tiles(cam, st, full, sample_begin=s, sample_count=1, threads=threads)
        S, Q = S + smp, Q + smp * smp
    return S, Q


def bars(values_a, values_b):
    sa, sb = max(values_a) - min(values_a), max(values_b) - min(values_b)
    return {"ratio_spread": sa, "ratio_bar": max(values_a) + 2.0 * sa, "spearman_spread": sb, "spearman_bar": min(values_b) - 2.0 * sb}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_atrous_dual", "atrous_dual_bars.json"))
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--levels", type=int, nargs="*", default=[])
    ap.add_argument("--ref-spp", type=int, default=REF_SPP)
    ap.add_argument("--seeds", type=int, default=3)
    a = ap.parse_args()
    cam = scenes.camera(W, H)
    tiles = generate_tiles(W, H, (32, 32))
    seeds = [scenes.SEED, scenes.SEED + 2, scenes.SEED + 3][: a.seeds]  # (SEED + 1 is the converged frame's)
    result = {"width": W, "height": H, "half_spp": HALF, "reference_spp": a.ref_spp, "levels": 5, "k": 3.0, "alpha": 1.0, "seeds": seeds, "scenes": {}}
    for which, sc in (("spheres", scenes.reflective_spheres()), ("mesh", scenes.gold_dragon_standin(n=24))):
        osc = oracle_lib.OracleScene(sc, fast=True)
        st_ref = Settings(cam, sample_count=a.ref_spp, bounce_limit=5, seed=scenes.SEED + 1)
        ref = osc.render_tiles(cam, st_ref, tiles, threads=a.threads) / float(a.ref_spp)
        rows = []
        for seed in seeds:
            S_a, Q_a = half_sums(osc, cam, seed, 0, a.threads)
            S_b, Q_b = half_sums(osc, cam, seed, HALF, a.threads)
            n = np.full((H, W), HALF)
            out, err = adref.atrous_dual(S_a, Q_a, S_b, Q_b, n, n)
            single = aref.atrous(S_a + S_b, Q_a + Q_b, 2 * n)
            row = {"seed": seed, "rmse_unfiltered": rmse((S_a + S_b) / (2.0 * HALF), ref), "rmse_dual": rmse(out, ref), "rmse_single": rmse(single, ref),
                   "sqrt_mean_err_over_rmse": float(np.sqrt(err.mean())) / rmse(out, ref),
                   "spearman": spearman(denoise_dual_ref.tile_error_dual(err, tiles), tile_true_rms(out, ref, tiles))}
            row["ratio"] = row["rmse_dual"] / row["rmse_single"]
            if a.levels:
                halves, dual = adref.filtered_halves_all(S_a, Q_a, S_b, Q_b, n, n, a.levels)
                row["by_levels"] = {}
                for lv in sorted(set(a.levels)):
                    o, e = denoise_dual_ref.combine(*halves[lv], S_a, S_b, n, n, dual)
                    row["by_levels"][str(lv)] = {"rmse_dual": rmse(o, ref), "spearman": spearman(denoise_dual_ref.tile_error_dual(e, tiles), tile_true_rms(o, ref, tiles))}
            rows.append(row)
            print(which, json.dumps(row), flush=True)
        result["scenes"][which] = {"rows": rows, **bars([r["ratio"] for r in rows], [r["spearman"] for r in rows])}
        print(which, json.dumps({k: v for k, v in result["scenes"][which].items() if k != "rows"}), flush=True)
        osc.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
