"""rmd_despike_dual restated in numpy scalars over tests/despike_ref.py's functions (include/raymond_hip.h has the definition): the merge as one np.float64
addition, the dual validity, rmd_despike's own planes, donor and test on the merged pixel, and the half-by-half copy.  np.float64 operations only.
`variant` makes one of four WRONG readings of the definition, which tests/test_despike_dual_host.py tells the right one from.  No GPU, no library."""
import numpy as np

import despike_ref

VARIANTS = ("per_half", "split_merged", "merged_counts", "merged_n_ge_2")


def merge(SA, QA, SB, QB):
    """(S, Q): one rounded addition per value."""
    with np.errstate(all="ignore"):
        return np.asarray(SA, dtype=np.float64) + np.asarray(SB, dtype=np.float64), np.asarray(QA, dtype=np.float64) + np.asarray(QB, dtype=np.float64)


def dual_planes(S, Q, n_a, n_b, variant=None):
    """(valid, Y, V) of the merged pixels: rmd_despike's planes at n_a + n_b, valid only where both halves hold a sample."""
    n = (n_a.astype(np.uint64) + n_b.astype(np.uint64)).astype(np.uint32)
    valid, Y, V = despike_ref.luminance_planes(S, Q, n)  # (n >= 2 and finite merged sums)
    if variant != "merged_n_ge_2":
        valid = valid & (n_a >= 1) & (n_b >= 1)
        Y = np.where(valid, Y, np.nan)
        V = np.where(valid, V, np.nan)
    return valid, Y, V


def take(out, src, x, y, qx, qy, n_p, n_q):
    """Half-plane `out` at (x, y) from `src` at the donor: its bits at equal counts, else its per-sample moment at n_p."""
    if n_p == n_q:
        out.view(np.uint64)[y, x] = src.view(np.uint64)[qy, qx]
    else:
        for c in range(3):
            out[y, x, c] = (src[qy, qx, c] / np.float64(n_q)) * np.float64(n_p)


def despike_dual(SA, QA, SB, QB, rects, counts_a, counts_b, radius=2, rank=2, k=6.0, ratio=2.0, floor=0.0, variant=None):
    """rmd_despike_dual: (S'_A, Q'_A, S'_B, Q'_B, replaced, spikes); spikes is the list of (x, y, donor x, donor y)."""
    SA, QA, SB, QB = (np.ascontiguousarray(a, dtype=np.float64) for a in (SA, QA, SB, QB))
    rects = list(rects)
    if variant == "per_half":  # WRONG: each half decides from its own samples
        oa = despike_ref.despike(SA, QA, rects, counts_a, radius, rank, k, ratio, floor)
        ob = despike_ref.despike(SB, QB, rects, counts_b, radius, rank, k, ratio, floor)
        return oa[0], oa[1], ob[0], ob[1], oa[2] + ob[2], sorted(set(oa[3]) | set(ob[3]))
    H, W = SA.shape[0], SA.shape[1]
    n_a, idx = despike_ref.count_image(W, H, rects, counts_a)
    n_b, _ = despike_ref.count_image(W, H, rects, counts_b)
    S, Q = merge(SA, QA, SB, QB)
    valid, Y, V = dual_planes(S, Q, n_a, n_b, variant)
    outs = [a.copy() for a in (SA, QA, SB, QB)]
    replaced = np.zeros(len(rects), dtype=np.uint32)
    spikes = []
    k, ratio, floor = np.float64(k), np.float64(ratio), np.float64(floor)
    k2 = k * k
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                if not valid[y, x]:
                    continue
                d = despike_ref.donor_of(valid, Y, x, y, radius, rank)
                if d is None:
                    continue
                qx, qy = d
                e = (Y[y, x] - ratio * Y[qy, qx]) - floor
                if not (e > 0.0 and e * e > k2 * V[qy, qx]):
                    continue
                spikes.append((x, y, qx, qy))
                replaced[idx[y, x]] += 1
                halves = ((outs[0], SA, n_a), (outs[1], QA, n_a), (outs[2], SB, n_b), (outs[3], QB, n_b))
                if variant == "split_merged":  # WRONG: the donor's merged sums, half to each half
                    for (out, _, _), M in zip(halves, (S, Q, S, Q)):
                        for c in range(3):
                            out[y, x, c] = M[qy, qx, c] * np.float64(0.5)
                elif variant == "merged_counts":  # WRONG: equal MERGED counts copy, others scale by the merged counts
                    n_p, n_q = int(n_a[y, x]) + int(n_b[y, x]), int(n_a[qy, qx]) + int(n_b[qy, qx])
                    for out, src, _ in halves:
                        take(out, src, x, y, qx, qy, n_p, n_q)
                else:
                    for out, src, n in halves:
                        take(out, src, x, y, qx, qy, int(n[y, x]), int(n[qy, qx]))
    return outs[0], outs[1], outs[2], outs[3], replaced, spikes


same_bits = despike_ref.same_bits
