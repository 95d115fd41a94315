"""rmd_tile_weighted_error and rmd_display_weights restated in numpy (include/raymond_hip.h has the definitions): np.float64 operations only — elementwise
array arithmetic is the same rounded IEEE operation per element, nothing fused —, the weight's index taken from the 64 bits of the luminance.  The rule is
here: the counter, E and the final step; a pixel's validity, Y and V and the kernel's summation order are tile_reduce_ref.py's.  No GPU, no library."""
import numpy as np

from tile_reduce_ref import A0, A1, A2, LANES, WAVE, WB, WG, WR, combine, moments, rect_sums, same_bits  # noqa: F401 — the order, and the names callers know

N_WEIGHTS = 260
BELOW, ABOVE, ZERO, NEGATIVE, NOT_FINITE = 256, 257, 258, 259, 260  # the luminance histogram's side counters, in its order

DTYPE = np.dtype([("rms", "<f8"), ("mean_weighted_variance", "<f8"), ("mean_luma", "<f8"), ("mean_variance", "<f8"), ("valid", "<u4"),
                  ("invalid", "<u4")])  # rmd_tile_weighted, field for field
FLOAT_FIELDS = ("rms", "mean_weighted_variance", "mean_luma", "mean_variance")


def counter(y):
    """The luminance histogram's counter of every double of `y`, from its bits alone: E the unbiased exponent, M the top two mantissa bits."""
    bits = np.ascontiguousarray(y, dtype=np.float64).view(np.uint64)
    mag = bits & np.uint64(0x7FFFFFFFFFFFFFFF)
    biased = (mag >> np.uint64(52)).astype(np.int64)
    k = (biased - (1023 - 32)) * 4 + ((mag >> np.uint64(50)) & np.uint64(3)).astype(np.int64)
    k = np.where(biased >= 1023 + 32, ABOVE, k)
    k = np.where(biased < 1023 - 32, BELOW, k)
    k = np.where((bits >> np.uint64(63)) != 0, NEGATIVE, k)
    k = np.where(mag == 0, ZERO, k)
    k = np.where(mag >= np.uint64(0x7FF0000000000000), NOT_FINITE, k)
    return k


def pixels(s, q, n, weights):
    """(valid, Y, V, E) of pixels whose sums are the rows of the (N, 3) arrays s and q, all at count n.  Y, V and E of a pixel that is not valid mean nothing."""
    s, q = np.asarray(s, dtype=np.float64).reshape(-1, 3), np.asarray(q, dtype=np.float64).reshape(-1, 3)
    weights = np.asarray(weights, dtype=np.float64)
    assert weights.shape == (N_WEIGHTS,)
    valid, Y, V = moments(s, q, n)
    with np.errstate(all="ignore"):
        k = counter(Y)
        valid = valid & (k < N_WEIGHTS)  # a luminance that is not finite: the pixel counts as invalid
        w = weights[np.minimum(k, N_WEIGHTS - 1)]
        E = np.where(w == 0.0, np.float64(0.0), w * V)  # one rounded product; a zero weight gives 0 even under V = +inf
    return valid, Y, V, E


def reduce_rect(valid, Y, V, E):
    """One rect from its pixels' values in the rect's row-major order: rmd_tile_weighted's fields as a tuple."""
    n_px = len(valid)
    if n_px == 0:
        return (0.0, 0.0, 0.0, 0.0, 0, 0)
    sums, n_valid = rect_sums(valid, Y, V, E)
    with np.errstate(all="ignore"):
        n_invalid = n_px - n_valid
        m = np.float64(n_valid)
        mean_y, mean_v, mean_e = [(s / m if n_valid else np.float64(0.0)) for s in sums]
        rms = np.sqrt(mean_e)
        if n_invalid:
            rms = np.float64(np.inf)
        if rms != rms:
            rms = np.float64(np.inf)
    return (rms, mean_e, mean_y, mean_v, n_valid, n_invalid)


def tile_weighted_error(S, Q, rects, counts, weights):
    """rmd_tile_weighted_error: a structured array (DTYPE) with one entry per rect of the (H, W, 3) sums S and sums of squares Q."""
    S, Q = np.ascontiguousarray(S, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
    out = np.zeros(len(rects), dtype=DTYPE)
    for j, ((l, t, w, h), n) in enumerate(zip(rects, counts)):
        s, q = S[t : t + h, l : l + w].reshape(-1, 3), Q[t : t + h, l : l + w].reshape(-1, 3)
        out[j] = reduce_rect(*pixels(s, q, int(n), weights))
    return out


def bin_centres():
    """The 256 bins' centres 2^E (1 + (M + 0.5) / 4), E = i // 4 - 32, M = i % 4: exact."""
    i = np.arange(256)
    return np.ldexp(1.0 + ((i % 4) + 0.5) * 0.25, i // 4 - 32)


def display_weights(exposure, gamma, display_floor):
    """rmd_display_weights: the squared slope of D(y) = (1 - exp(-y e))^(1/g) per counter, capped at the luminance that displays at display_floor."""
    e, g, f = np.float64(exposure), np.float64(gamma), np.float64(display_floor)
    with np.errstate(all="ignore"):
        y_floor = -np.log1p(-np.power(f, g)) / e

        def slope2(y):
            t = -np.expm1(-y * e)
            s = (np.float64(1.0) / g) * np.power(t, np.float64(1.0) / g - np.float64(1.0)) * e * np.exp(-y * e)
            w = s * s
            w = np.where(np.isnan(w), 0.0, w)
            return np.minimum(w, np.finfo(np.float64).max)

        out = np.zeros(N_WEIGHTS, dtype=np.float64)
        out[:256] = slope2(np.maximum(bin_centres(), y_floor))
        out[BELOW] = out[ZERO] = out[NEGATIVE] = slope2(y_floor)
        out[ABOVE] = slope2(np.float64(2.0**32))
    return out, y_floor
