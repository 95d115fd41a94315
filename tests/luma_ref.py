"""numpy restatement of rmd_luminance_histogram_tiles and a Python one of rmd_exposure_from_histogram (include/raymond_hip.h states both), and the
values the binning is tried on — the ones tests/luma_bins_main.cpp uses.

The histogram: for a packed pixel of rect j, s = the sum (np.add of the two buffers, computed once in float64, when there are two), p = s / count_j,
Y = (0.2126 * p_0 + 0.7152 * p_1) + 0.0722 * p_2 — numpy rounds every elementwise operation by itself, so no multiply-add is fused —, and the counter is
read from Y's bits through view(np.uint64).  Rects are counted in order, an overlap twice."""
import math

import numpy as np

from raymond_amd import abi, render

BINS = abi.RMD_LUMA_BINS
BELOW, ABOVE, ZERO, NEGATIVE, NOT_FINITE = 256, 257, 258, 259, 260
COEF = (0.2126, 0.7152, 0.0722)


def luminance(p):
    """(..., 3) radiances -> (...) luminances."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(all="ignore"):
        return (np.float64(COEF[0]) * p[..., 0] + np.float64(COEF[1]) * p[..., 1]) + np.float64(COEF[2]) * p[..., 2]


def counter_of(y):
    """The counter (0 .. 260) of every luminance, from its bits."""
    bits = np.ascontiguousarray(y, dtype=np.float64).view(np.uint64)
    mag = bits & np.uint64(0x7FFFFFFFFFFFFFFF)
    biased = (mag >> np.uint64(52)).astype(np.int64)
    top2 = ((mag >> np.uint64(50)) & np.uint64(3)).astype(np.int64)
    out = (biased - 991) * 4 + top2  # E + 32 = biased - 1023 + 32
    out = np.where(biased < 991, BELOW, out)
    out = np.where(biased >= 1055, ABOVE, out)
    out = np.where((bits >> np.uint64(63)) != 0, NEGATIVE, out)
    out = np.where(mag == 0, ZERO, out)
    out = np.where(mag >= np.uint64(0x7FF0000000000000), NOT_FINITE, out)
    return out


def rect_luminances(acc, rects, counts, second=None):
    """The luminance of every packed pixel, rect after rect, as one flat array."""
    acc = np.asarray(acc, dtype=np.float64)
    with np.errstate(all="ignore"):
        total = acc if second is None else np.add(acc, np.asarray(second, dtype=np.float64))
    ys = []
    for (l, t, w, h), c in zip(rects, counts):
        with np.errstate(all="ignore"):
            p = total[t : t + h, l : l + w] / np.float64(c)
        ys.append(luminance(p).reshape(-1))
    return np.concatenate(ys) if ys else np.zeros(0)


def histogram(acc, rects, counts, second=None):
    """render.LumaHistogram of the (H, W, 3) sums `acc` (+ `second`) over `rects`, rect i at counts[i]."""
    y = rect_luminances(acc, rects, counts, second)
    n = np.bincount(counter_of(y), minlength=261).astype(np.uint64)
    return render.LumaHistogram(n[:BINS], int(n[BELOW]), int(n[ABOVE]), int(n[ZERO]), int(n[NEGATIVE]), int(n[NOT_FINITE]), int(y.size))


def exposure(hist, percentile=0.99, target=0.8):
    """rmd_exposure_from_histogram, restated with math.ceil, math.ldexp and math.log1p."""
    n = int(hist.below) + sum(int(v) for v in hist.bins) + int(hist.above)
    if n == 0:
        return 1.0
    r = min(max(math.ceil(percentile * float(n)), 1), n)
    seen = int(hist.below)
    y = 2.0**-32
    if seen < r:
        y = 2.0**32
        for i in range(BINS):
            seen += int(hist.bins[i])
            if seen >= r:
                y = math.ldexp(1.0 + (i % 4 + 1) * 0.25, i // 4 - 32)
                break
    return -math.log1p(-target) / y


# ---------------------------------------------------------------- the values of tests/luma_bins_main.cpp
def edge_values():
    """Every bin edge ldexp(1 + m / 4, e), e in -34 .. 33, with the doubles just below and just above it."""
    out = []
    for e in range(-34, 34):
        for m in range(4):
            edge = math.ldexp(1.0 + m / 4.0, e)
            out += [edge, float(np.nextafter(edge, 0.0)), float(np.nextafter(edge, np.inf))]
    return out


SPECIAL_BITS = (0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x8000000000000001, 0x800FFFFFFFFFFFFF,
                0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0x7FF0000000000001,
                0xFFF0000000000001, 0x7FF7FFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF,
                0x0010000000000000, 0x7FEFFFFFFFFFFFFF, 0x8010000000000000, 0xFFEFFFFFFFFFFFFF, 0xBFF0000000000000)  # DBL_MIN, DBL_MAX, their negatives, -1


def special_values():
    return np.array(SPECIAL_BITS, dtype=np.uint64).view(np.float64)


def radiance_with_luminance(v):
    """A radiance (p_0, p_1, p_2) whose luminance is EXACTLY the positive finite double v: one channel x with fl(coefficient * x) == v and the other two 0
    (the additions of zeros are exact).  None when no channel reaches v (x steps the product by 0.6 - 1.7 ulps of v, depending on the channel)."""
    v = np.float64(v)
    for ch in (1, 0, 2):
        x0 = v / np.float64(COEF[ch])
        lo = hi = x0
        cands = [x0]
        for _ in range(6):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            cands += [lo, hi]
        for x in cands:
            if np.float64(COEF[ch]) * x == v:
                p = [0.0, 0.0, 0.0]
                p[ch] = float(x)
                return p
    return None


def sum_for(p, count):
    """A sum s with fl(s / count) == p where there is one near p * count (else p * count itself); count 0: the value itself."""
    p = np.float64(p)
    if count == 0 or not np.isfinite(p) or p == 0.0:
        return float(p)
    with np.errstate(all="ignore"):
        s0 = p * np.float64(count)
        lo = hi = s0
        cands = [s0]
        for _ in range(3):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            cands += [lo, hi]
        for s in cands:
            if s / np.float64(count) == p:
                return float(s)
    return float(s0)
