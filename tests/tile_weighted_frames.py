"""The frames, weight tables and rect lists tests/test_gpu_tile_weighted.py sends to rmd_tile_weighted_error; tests/test_tile_weighted_host.py checks on the
CPU that each class is what it names.  The rect lists are tests/tile_luma_frames.py's: the two kernels share the striding and the combine.

A note on the "saturated" class.  The per-pixel step guards a zero weight against V = +inf (0 * inf would be NaN), but no VALID pixel reaches V = +inf: its
sums are finite, s * u >= 0, so (q - s u) / (n - 1) <= q, v <= q / 2 and V <= 0.57 * q / 2 is finite.  The class therefore holds the largest V finite sums
give (about 5e307) under a zero weight — the tile's rms is exactly 0 — and, under a weight of 1e30, the overflow of w * V to +inf, which is the rms then.
tests/tile_weighted_rule_main.cpp calls the per-pixel step itself with V = +inf and w = 0."""
import numpy as np

import tile_luma_frames as luma_frames
import tile_weighted_ref as ref

W, H, NMAX = luma_frames.W, luma_frames.H, luma_frames.NMAX
RECTS, WIDE, WIDE_RECTS = luma_frames.RECTS, luma_frames.WIDE, luma_frames.WIDE_RECTS
BAD_PIXEL, BAD_RECT = luma_frames.BAD_PIXEL, luma_frames.BAD_RECT
rects_and_counts, random_positive, permuted_tile = luma_frames.rects_and_counts, luma_frames.random_positive, luma_frames.permuted_tile
ORDER_SEED = 11  # permuted_tile's seed at which the 32 x 32 tile's sums change their bits under the "ones" and the "random" table (two orders often agree by chance)
SEAM_RECT = 1  # the 16 x 16 rect at count 2: u = s / 2 is exact, so its pixels' luminances are exactly the ones the "edges" class plants
WEIGHTS = (np.float64(0.2126), np.float64(0.7152), np.float64(0.0722))


def _planted(target):
    """(channel, u) with fl(weight[channel] * u) == target exactly, searched among the doubles next to target / weight; None if there is none."""
    for c in (1, 0, 2):
        u = np.float64(target) / WEIGHTS[c]
        for cand in np.concatenate([[u], *[[a, b] for a, b in zip(_walk(u, +1, 40), _walk(u, -1, 40))]]):
            if WEIGHTS[c] * cand == target:
                return c, np.float64(cand)
    return None


def _walk(x, direction, steps):
    out = []
    for _ in range(steps):
        x = np.nextafter(x, np.inf * direction)
        out.append(x)
    return out


def edge_targets():
    """[(edge index 0 .. 256, under, target luminance, (channel, u))]: every bin's lower edge (256: 2^32, where `above` begins) and the double one ulp under
    it, for which a one-channel pixel with exactly that luminance exists."""
    out = []
    for i in range(257):
        edge = np.ldexp(1.0 + (i % 4) * 0.25, i // 4 - 32)
        for under in (0, 1):
            target = np.nextafter(edge, 0.0) if under else edge
            found = _planted(target)
            if found is not None:
                out.append((i, under, target, found))
    return out


_EDGES = None


def edges_frame(width=W, height=H, n=2):
    """Pixel p (row-major over the frame) holds target p % len(targets) at count n: one channel lit, S = u * n (exact for n = 2), Q = 0.75 S^2."""
    global _EDGES
    if _EDGES is None:
        _EDGES = edge_targets()
    S = np.zeros((height, width, 3))
    flat = S.reshape(-1, 3)
    for p in range(len(flat)):
        _, _, _, (c, u) = _EDGES[p % len(_EDGES)]
        flat[p, c] = u * np.float64(n)
    return S, S * S * 0.75


def zeros_frame(width=W, height=H):
    """Zeros of both signs and negative sums, pixel by pixel in turn: +0 (Y = +0), -0 (Y = -0), all negative (Y < 0), and a positive pixel."""
    S, Q = random_positive(width, height, seed=7)
    kind = np.arange(width * height).reshape(height, width) % 4
    S[kind == 0] = 0.0
    S[kind == 1] = -0.0
    S[kind == 2] *= -1.0
    Q[kind <= 1] = 0.0
    return S, Q


def saturated_frame(width=W, height=H):
    """Every pixel's luminance at 2^40 and above (the `above` counter) with Q near the largest double: V is about 5e307, the largest finite sums give."""
    rng = np.random.default_rng(11)
    S = rng.uniform(1.0, 2.0, (height, width, 3)) * 2.0**75  # at the count 2^32 - 1 the mean is still 2^43
    Q = np.full((height, width, 3), 1.7e308)
    return S, Q


def frames():
    """name -> (S, Q) on the W x H frame."""
    S, Q = random_positive()
    out = {"random": (S, Q)}
    out["tiny"] = (S * 2.0**-500, Q * 2.0**-1000)  # every luminance below 2^-32
    out["huge"] = (S * 2.0**500, Q * 2.0**1000)  # ... at or over 2^32
    out["edges"] = edges_frame()
    out["zeros"] = zeros_frame()
    out["saturated"] = saturated_frame()
    nan_S = S.copy()
    nan_S[BAD_PIXEL[1], BAD_PIXEL[0], 1] = np.nan
    out["nan_in_S"] = (nan_S, Q)
    inf_Q = Q.copy()
    inf_Q[BAD_PIXEL[1], BAD_PIXEL[0], 2] = np.inf
    out["inf_in_Q"] = (S, inf_Q)
    return out


ONE_BIN = 130  # [2^0.5 .. ): the bin of luminances in [1.5, 1.75), which the random frame's means at count 17 reach


def tables():
    """name -> 260 weights.  "one_bin" is 0 except one bin: a lookup with a wrong index gives another sum."""
    rng = np.random.default_rng(13)
    one = np.zeros(ref.N_WEIGHTS)
    one[ONE_BIN] = 3.0
    return {
        "ones": np.ones(ref.N_WEIGHTS),
        "random": rng.uniform(0.0, 4.0, ref.N_WEIGHTS) * (rng.uniform(size=ref.N_WEIGHTS) > 0.2),  # a fifth of the entries exactly 0
        "display_1": ref.display_weights(1.0, 2.2, 1.0 / 255.0)[0],
        "display_0.001": ref.display_weights(0.001, 2.2, 1.0 / 255.0)[0],
        "one_bin": one,
        "zero": np.zeros(ref.N_WEIGHTS),
        "big": np.full(ref.N_WEIGHTS, 1e30),
    }
