"""What the numpy restatements of the per-tile measures (tile_luma_ref.py, tile_weighted_ref.py) restate alike: a pixel's validity, Y and V, and the kernels'
summation order — 256 lanes that each add their pixels in order, and the combine spelt out (raymond_amd/csrc/tile_reduce.hpp has the order).  np.float64
operations only: elementwise array arithmetic is the same rounded IEEE operation per element, nothing fused.  No GPU, no library."""
import numpy as np

WR, WG, WB = np.float64(0.2126), np.float64(0.7152), np.float64(0.0722)
A0, A1, A2 = WR * WR, WG * WG, WB * WB  # the binary64 product of each weight with itself
LANES, WAVE = 256, 64


def moments(s, q, n):
    """(valid, Y, V) of pixels whose sums are the rows of the (N, 3) float64 arrays s and q, all at count n.  Y and V of a pixel that is not valid mean nothing."""
    with np.errstate(all="ignore"):
        valid = (np.isfinite(s).all(axis=1) & np.isfinite(q).all(axis=1)) if n >= 2 else np.zeros(len(s), dtype=bool)
        nd = np.float64(n)
        u = s / nd
        t = (q - s * u) / (nd - np.float64(1.0))
        t = np.where(t > 0.0, t, np.float64(0.0))
        v = t / nd
        Y = (WR * u[:, 0] + WG * u[:, 1]) + WB * u[:, 2]
        V = (A0 * v[:, 0] + A1 * v[:, 1]) + A2 * v[:, 2]
    return valid, Y, V


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


def rect_sums(valid, *values):
    """One rect (at least one pixel) from its pixels' values in the rect's row-major order: the lane-ordered sum of each of `values` over the valid pixels,
    as a list, and the valid count."""
    n_px = len(valid)
    rows = -(-n_px // LANES)
    pad = rows * LANES - n_px
    grid = lambda a, fill: np.concatenate([a, np.full(pad, fill, dtype=a.dtype)]).reshape(rows, LANES)  # noqa: E731 — [k, t] is pixel t + 256 k
    ok = grid(valid, False)
    sums = []
    with np.errstate(all="ignore"):
        for vals in values:
            vals, acc = grid(vals, np.float64(0.0)), np.zeros(LANES, dtype=np.float64)
            for k in range(rows):  # lane t meets its pixels in the order t, t + 256, ...
                acc = np.where(ok[k], acc + vals[k], acc)
            sums.append(combine(acc))
        return sums, int(combine(ok.sum(axis=0).astype(np.uint32)))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))
