"""rmd_tile_luma_error restated in numpy (include/raymond_hip.h has the definition): np.float64 operations only — elementwise array arithmetic is the same
rounded IEEE operation per element, nothing fused.  The rule is here: d, R and the final step; a pixel's validity, Y and V and the kernel's summation order
are tile_reduce_ref.py's.  No GPU, no library."""
import numpy as np

from tile_reduce_ref import A0, A1, A2, LANES, WAVE, WB, WG, WR, combine, moments, rect_sums, same_bits  # noqa: F401 — the order, and the names callers know

DTYPE = np.dtype([("tile_rms", "<f8"), ("pixel_rms", "<f8"), ("mean_luma", "<f8"), ("mean_variance", "<f8"), ("mean_rel_variance", "<f8"), ("valid", "<u4"),
                  ("invalid", "<u4")])  # rmd_tile_luma, field for field
FLOAT_FIELDS = ("tile_rms", "pixel_rms", "mean_luma", "mean_variance", "mean_rel_variance")


def pixels(s, q, n, floor):
    """(valid, Y, V, R) of pixels whose sums are the rows of the (N, 3) arrays s and q, all at count n.  Y, V and R of a pixel that is not valid mean nothing."""
    s, q = np.asarray(s, dtype=np.float64).reshape(-1, 3), np.asarray(q, dtype=np.float64).reshape(-1, 3)
    floor = np.float64(floor)
    valid, Y, V = moments(s, q, n)
    with np.errstate(all="ignore"):
        d = np.abs(Y)
        d = np.where(d > floor, d, floor)
        R = (V / d) / d
    return valid, Y, V, R


def reduce_rect(valid, Y, V, R, floor):
    """One rect from its pixels' values in the rect's row-major order: rmd_tile_luma's fields as a tuple."""
    n_px = len(valid)
    if n_px == 0:
        return (0.0, 0.0, 0.0, 0.0, 0.0, 0, 0)
    floor = np.float64(floor)
    sums, n_valid = rect_sums(valid, Y, V, R)
    with np.errstate(all="ignore"):
        n_invalid = n_px - n_valid
        m = np.float64(n_valid)
        mean_y, mean_v, mean_r = [(s / m if n_valid else np.float64(0.0)) for s in sums]
        D = np.abs(mean_y)
        if not D > floor:
            D = floor
        tile_rms, pixel_rms = np.sqrt(mean_v) / D, np.sqrt(mean_r)
        if n_invalid:
            tile_rms = pixel_rms = np.float64(np.inf)
        if tile_rms != tile_rms:
            tile_rms = np.float64(np.inf)
        if pixel_rms != pixel_rms:
            pixel_rms = np.float64(np.inf)
    return (tile_rms, pixel_rms, mean_y, mean_v, mean_r, n_valid, n_invalid)


def tile_luma_error(S, Q, rects, counts, floor):
    """rmd_tile_luma_error: a structured array (DTYPE) with one entry per rect of the (H, W, 3) sums S and sums of squares Q."""
    S, Q = np.ascontiguousarray(S, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
    out = np.zeros(len(rects), dtype=DTYPE)
    for j, ((l, t, w, h), n) in enumerate(zip(rects, counts)):
        s, q = S[t : t + h, l : l + w].reshape(-1, 3), Q[t : t + h, l : l + w].reshape(-1, 3)
        out[j] = reduce_rect(*pixels(s, q, int(n), floor), floor)
    return out
