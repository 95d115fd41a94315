"""rmd_tile_error and rmd_tile_error_dual restated in numpy, operation for operation (include/raymond_hip.h states both).  numpy rounds every elementwise
operation by itself, so no multiply-add is fused and every step is the rounded binary64 one.  No GPU, no library.

rmd_tile_error: m = S / n; v = (Q - S*m) / (n - 1), 0 if negative; e_c = sqrt(v / n) / max(|m|, floor); the pixel's error is its largest e_c, +inf with a
non-finite S or Q or n < 2; the rect's is its largest pixel's, 0 without pixels (also with n < 2: there is no pixel to be +inf).

rmd_tile_error_dual: the header's sum order, literally.  The rect's pixels numbered row-major and padded with +0.0 to a multiple of 256 (a partial sum starts
at +0.0 and can never become -0.0, so adding +0.0 changes no bit); the rows of the (-1, 256) view are added in order into 256 partial sums, a NaN skipped and
remembered; then t with t ^ 32, ^ 16, ... ^ 1 within each group of 64; then (g0 + g1) + (g2 + g3).  sqrt(total / pixels), +inf after a NaN, 0 without pixels."""
import numpy as np

LANES = 256


def pixel_errors(S, Q, n, floor):
    """The (H, W) map of e_pixel before any rect's maximum."""
    S, Q = np.asarray(S, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    nd = np.float64(n)
    with np.errstate(all="ignore"):
        m = S / nd
        v = (Q - S * m) / (nd - np.float64(1.0))
        v = np.where(v < 0.0, np.float64(0.0), v)
        e = np.sqrt(v / nd) / np.maximum(np.abs(m), np.float64(floor))
        ep = e.max(axis=2)
    bad = ~(np.isfinite(S).all(axis=2) & np.isfinite(Q).all(axis=2))
    if n < 2:
        bad[:] = True
    return np.where(bad, np.inf, ep)


def rect_maxima(pixel_map, rects):
    """Per rect the largest value of an (H, W) map, 0 for a rect without pixels."""
    out = np.zeros(len(rects))
    for j, (l, t, w, h) in enumerate(rects):
        if w * h:
            out[j] = pixel_map[t : t + h, l : l + w].max()
    return out


def tile_error(S, Q, n, floor, rects):
    """rmd_tile_error: one float64 per rect."""
    return rect_maxima(pixel_errors(S, Q, n, floor), rects)


def partial_sums(values):
    """(the 256 partial sums, whether a NaN was skipped) of a flat array: partial sum t adds values t, t + 256, t + 512, ... in that order."""
    values = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    rows = np.concatenate([values, np.zeros(-values.size % LANES)]).reshape(-1, LANES)
    s = np.zeros(LANES)
    nan = np.isnan(rows)
    with np.errstate(all="ignore"):
        for row, skip in zip(rows, nan):
            s = np.where(skip, s, s + row)
    return s, bool(nan.any())


def halving_total(partials):
    """The 256 partial sums added pairwise: t with t ^ 32, ^ 16, ... ^ 1 within each group of 64 (every lane adds, lane 0 of the group holds the group's
    sum), then (g0 + g1) + (g2 + g3)."""
    lane = np.arange(LANES)
    s = np.asarray(partials, dtype=np.float64)
    with np.errstate(all="ignore"):
        for off in (32, 16, 8, 4, 2, 1):
            s = s + s[lane ^ off]
        return float((s[0] + s[64]) + (s[128] + s[192]))


def ordered_sum(values):
    """(total, whether a NaN was skipped) of a flat array in the header's order."""
    s, nan = partial_sums(values)
    return halving_total(s), nan


def rect_values(err, rect):
    l, t, w, h = rect
    return np.asarray(err, dtype=np.float64)[t : t + h, l : l + w].reshape(-1)


def ordered_total(err, rect):
    """The header's sum of the (H, W) image `err` over `rect`, NaNs skipped."""
    return ordered_sum(rect_values(err, rect))[0]


def tile_error_dual(err, rects):
    """rmd_tile_error_dual: one float64 per rect."""
    out = np.zeros(len(rects))
    for j, rect in enumerate(rects):
        n_px = rect[2] * rect[3]
        if n_px == 0:
            continue
        total, nan = ordered_sum(rect_values(err, rect))
        with np.errstate(all="ignore"):
            out[j] = np.inf if nan else np.sqrt(np.float64(total) / np.float64(n_px))
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def ulp_distance(a, b):
    """The number of doubles between finite a and b of the same sign (elementwise)."""
    ia = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    ib = np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return np.abs(ia - ib)
