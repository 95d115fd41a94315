"""rmd_tile_weighted_error_dual restated in numpy (include/raymond_hip.h has the definition): np.float64 operations only — elementwise array arithmetic is
the same rounded IEEE operation per element, nothing fused —, the weight's index taken from the 64 bits of the luminance as tests/tile_weighted_ref.py takes
it.  The rule is here: a pixel's validity, the luminance of its filtered means, E; the summation order is tile_reduce_ref.py's and the final step
tile_weighted_ref.py's.  Also rmd_tile_error_dual's definition, restated plainly, for the tie between the two.  No GPU, no library."""
import numpy as np

import tile_weighted_ref as weighted
from tile_reduce_ref import LANES, WB, WG, WR, combine, rect_sums, same_bits  # noqa: F401 — the order, and the names callers know

N_WEIGHTS, DTYPE, FLOAT_FIELDS = weighted.N_WEIGHTS, weighted.DTYPE, weighted.FLOAT_FIELDS


def pixels(o, e, weights):
    """(valid, Y, e, E) of pixels whose filtered means are the rows of the (N, 3) array o and whose error estimates are e.  Y and E of a pixel that is not
    valid mean nothing."""
    o, e = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(e, dtype=np.float64).reshape(-1)
    weights = np.asarray(weights, dtype=np.float64)
    assert weights.shape == (N_WEIGHTS,)
    with np.errstate(all="ignore"):
        valid = ~np.isnan(e) & np.isfinite(o).all(axis=1)  # e = +inf is valid, a negative e too
        Y = (WR * o[:, 0] + WG * o[:, 1]) + WB * o[:, 2]
        k = weighted.counter(Y)
        valid = valid & (k < N_WEIGHTS)  # a luminance that overflowed: the pixel counts as invalid
        w = weights[np.minimum(k, N_WEIGHTS - 1)]
        E = np.where(w == 0.0, np.float64(0.0), w * e)  # one rounded product; a zero weight gives 0 even under e = +inf
    return valid, Y, e, E


def tile_weighted_error_dual(out, err, rects, weights, pixels=pixels):
    """rmd_tile_weighted_error_dual: a structured array (DTYPE) with one entry per rect of the (H, W, 3) filtered means `out` and the (H, W) image `err`."""
    out, err = np.ascontiguousarray(out, dtype=np.float64), np.ascontiguousarray(err, dtype=np.float64)
    res = np.zeros(len(rects), dtype=DTYPE)
    for j, (l, t, w, h) in enumerate(rects):
        res[j] = weighted.reduce_rect(*pixels(out[t : t + h, l : l + w].reshape(-1, 3), err[t : t + h, l : l + w].reshape(-1), weights))
    return res


def tile_error_dual(err, rects):
    """rmd_tile_error_dual's definition, read plainly: (result, radicand) per rect — sqrt(sum / pixels) with lane t adding its pixels t, t + 256, ... that are
    not NaN and the 256 partials combined; +inf (radicand NaN here) where an err of the rect is NaN; 0 for a rect without pixels."""
    err = np.ascontiguousarray(err, dtype=np.float64)
    res, rad = np.zeros(len(rects)), np.zeros(len(rects))
    for j, (l, t, w, h) in enumerate(rects):
        e = err[t : t + h, l : l + w].reshape(-1)
        if len(e) == 0:
            continue
        if np.isnan(e).any():
            res[j], rad[j] = np.inf, np.nan
            continue
        rows = -(-len(e) // LANES)
        grid = np.concatenate([e, np.zeros(rows * LANES - len(e))]).reshape(rows, LANES)
        live = (np.arange(rows * LANES) < len(e)).reshape(rows, LANES)
        acc = np.zeros(LANES)
        with np.errstate(all="ignore"):
            for k in range(rows):
                acc = np.where(live[k], acc + grid[k], acc)
            rad[j] = combine(acc) / np.float64(len(e))
            res[j] = np.sqrt(rad[j])
    return res, rad
