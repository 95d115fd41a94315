"""The (out, err) frames, weight tables and rect lists tests/test_gpu_tile_weighted_dual.py sends to rmd_tile_weighted_error_dual;
tests/test_tile_weighted_dual_host.py checks on the CPU that each class is what it names.  `out` is a filtered frame's means, (H, W, 3); `err` the dual
filter's error image, (H, W).  The rect lists are tests/tile_luma_frames.py's (their counts are not used: the measure reads none) and the tables
tests/tile_weighted_frames.py's: the kernels share the striding, the combine and the lookup."""
import numpy as np

import tile_luma_frames as luma_frames
import tile_weighted_frames as weighted_frames

W, H = luma_frames.W, luma_frames.H
RECTS = [r for r, _ in luma_frames.RECTS]
WIDE = luma_frames.WIDE
WIDE_RECTS = [r for r, _ in luma_frames.WIDE_RECTS]
BAD_PIXEL, BAD_RECT = luma_frames.BAD_PIXEL, luma_frames.BAD_RECT
TILE_RECT = 3  # the 32 x 32 rect: the adaptive check's tile, four pixels a lane
NEG_RECT = 14  # the 8 x 8 rect whose err the "negative_err" class makes negative
ONE_BIN = weighted_frames.ONE_BIN
INF_MEAN = 0.3  # the grey mean of the "inf_err" class's infinite pixels: its luminance is far from ONE_BIN's [1.5, 1.75)
ORDER_SEED = 285  # permuted()'s seed at which the 32 x 32 tile's sums change their bits under the "ones" and the "random" table (two orders often agree by chance; the host test holds that this one does not)
tables, edge_targets = weighted_frames.tables, weighted_frames.edge_targets


def random_positive(width=W, height=H, seed=1):
    """Means in (0.05, 2) a channel — luminances that reach ONE_BIN — and an err of the size a squared half-difference has at a few dozen samples."""
    rng = np.random.default_rng(seed)
    out = rng.uniform(0.05, 2.0, (height, width, 3))
    err = rng.uniform(0.1, 4.0, (height, width)) * 1e-3
    return out, err


_EDGES = None


def edges_frame(width=W, height=H):
    """Pixel p (row-major over the frame) holds target p % len(targets) as a one-channel MEAN u with fl(weight * u) == target; the other two channels are
    +0, so Y is the target exactly: every bin edge and the double under it."""
    global _EDGES
    if _EDGES is None:
        _EDGES = edge_targets()
    out, err = random_positive(width, height, seed=3)
    out[:] = 0.0
    flat = out.reshape(-1, 3)
    for p in range(len(flat)):
        _, _, _, (c, u) = _EDGES[p % len(_EDGES)]
        flat[p, c] = u
    return out, err


def zeros_frame(width=W, height=H):
    """Means +0 (Y = +0), -0 (Y = -0), all negative (Y < 0) and positive, pixel by pixel in turn."""
    out, err = random_positive(width, height, seed=7)
    kind = np.arange(width * height).reshape(height, width) % 4
    out[kind == 0] = 0.0
    out[kind == 1] = -0.0
    out[kind == 2] *= -1.0
    return out, err


def inf_err_frame(width=W, height=H):
    """err = +inf on every fourth pixel (row-major over the frame), whose means are the grey INF_MEAN: valid pixels outside ONE_BIN."""
    out, err = random_positive(width, height)
    fourth = np.arange(width * height).reshape(height, width) % 4 == 0
    err[fourth] = np.inf
    out[fourth] = INF_MEAN
    return out, err


def frames():
    """name -> (out, err) on the W x H frame."""
    out, err = random_positive()
    res = {"random": (out, err)}
    res["tiny"] = (out * 2.0**-500, err * 2.0**-1000)  # every luminance below 2^-32
    res["huge"] = (out * 2.0**500, err * 2.0**1000)  # ... at or over 2^32
    res["edges"] = edges_frame()
    res["zeros"] = zeros_frame()
    res["inf_err"] = inf_err_frame()
    x, y = BAD_PIXEL
    nan_err = err.copy()
    nan_err[y, x] = np.nan
    res["nan_err"] = (out, nan_err)
    nan_out = out.copy()
    nan_out[y, x, 1] = np.nan
    res["nan_out"] = (nan_out, err)
    inf_out = out.copy()
    inf_out[y, x, 2] = np.inf
    res["inf_out"] = (inf_out, err)
    neg = err.copy()
    l, t, w, h = RECTS[NEG_RECT]
    neg[t : t + h, l : l + w] *= -1.0
    res["negative_err"] = (out, neg)
    return res


INVALID_CLASSES = ("nan_err", "nan_out", "inf_out")  # the classes with the one invalid pixel at BAD_PIXEL


def wide_frame():
    """The 300 x 300 frame of WIDE_RECTS: a row longer than a wave and a column longer than the workgroup."""
    return random_positive(WIDE, WIDE, seed=9)


def permuted(out, err, rect, seed=ORDER_SEED):
    """The frame with the pixels of `rect` permuted among themselves, out and err together: tile_luma_frames.permuted_tile, err riding as three equal channels."""
    out2, err2 = luma_frames.permuted_tile(out, np.repeat(err[:, :, None], 3, axis=2), rect, seed)
    return out2, np.ascontiguousarray(err2[:, :, 0])
