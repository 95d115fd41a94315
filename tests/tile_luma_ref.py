"""rmd_tile_luma_error restated in numpy (include/raymond_hip.h has the definition): np.float64 operations only — elementwise array arithmetic is the same
rounded IEEE operation per element, nothing fused —, 256 lanes that each add their pixels in order, and the kernel's combine spelt out.  No GPU, no library."""
import numpy as np

WR, WG, WB = np.float64(0.2126), np.float64(0.7152), np.float64(0.0722)
A0, A1, A2 = WR * WR, WG * WG, WB * WB  # the binary64 product of each weight with itself
LANES, WAVE = 256, 64

DTYPE = np.dtype([("tile_rms", "<f8"), ("pixel_rms", "<f8"), ("mean_luma", "<f8"), ("mean_variance", "<f8"), ("mean_rel_variance", "<f8"), ("valid", "<u4"),
                  ("invalid", "<u4")])  # rmd_tile_luma, field for field
FLOAT_FIELDS = ("tile_rms", "pixel_rms", "mean_luma", "mean_variance", "mean_rel_variance")


def pixels(s, q, n, floor):
    """(valid, Y, V, R) of pixels whose sums are the rows of the (N, 3) arrays s and q, all at count n.  Y, V and R of a pixel that is not valid mean nothing."""
    s, q = np.asarray(s, dtype=np.float64).reshape(-1, 3), np.asarray(q, dtype=np.float64).reshape(-1, 3)
    floor = np.float64(floor)
    with np.errstate(all="ignore"):
        valid = (np.isfinite(s).all(axis=1) & np.isfinite(q).all(axis=1)) if n >= 2 else np.zeros(len(s), dtype=bool)
        nd = np.float64(n)
        u = s / nd
        t = (q - s * u) / (nd - np.float64(1.0))
        t = np.where(t > 0.0, t, np.float64(0.0))
        v = t / nd
        Y = (WR * u[:, 0] + WG * u[:, 1]) + WB * u[:, 2]
        V = (A0 * v[:, 0] + A1 * v[:, 1]) + A2 * v[:, 2]
        d = np.abs(Y)
        d = np.where(d > floor, d, floor)
        R = (V / d) / d
    return valid, Y, V, R


def combine(partials):
    """256 lane partials -> one value, as the kernel adds them: within each wave of 64 the lanes 32 apart, then 16, 8, 4, 2, 1; then (w0 + w1) + (w2 + w3)."""
    p = np.array(partials).reshape(LANES // WAVE, WAVE)
    lane = np.arange(WAVE)
    off = WAVE // 2
    with np.errstate(all="ignore"):
        while off:
            p = p + p[:, lane ^ off]
            off //= 2
        return (p[0, 0] + p[1, 0]) + (p[2, 0] + p[3, 0])


def reduce_rect(valid, Y, V, R, floor):
    """One rect from its pixels' values in the rect's row-major order: rmd_tile_luma's fields as a tuple."""
    n_px = len(valid)
    if n_px == 0:
        return (0.0, 0.0, 0.0, 0.0, 0.0, 0, 0)
    floor = np.float64(floor)
    rows = -(-n_px // LANES)
    pad = rows * LANES - n_px
    grid = lambda a, fill: np.concatenate([a, np.full(pad, fill, dtype=a.dtype)]).reshape(rows, LANES)  # noqa: E731 — [k, t] is pixel t + 256 k
    ok = grid(valid, False)
    sums = []
    with np.errstate(all="ignore"):
        for values in (Y, V, R):
            vals, acc = grid(values, np.float64(0.0)), np.zeros(LANES, dtype=np.float64)
            for k in range(rows):  # lane t meets its pixels in the order t, t + 256, ...
                acc = np.where(ok[k], acc + vals[k], acc)
            sums.append(combine(acc))
        n_valid = int(combine(ok.sum(axis=0).astype(np.uint32)))
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


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))
